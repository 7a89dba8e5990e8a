// Stand-alone host build of csrc/groth16.h for tests/test_groth16_native.py: the readers of the
// r1cs, the prepared powers-of-tau file and the Groth16 zkey, and the whole host path of setup
// and contribute, compiled with -fsanitize=address,undefined. stdin, one request per line:
//   setup <hex r1cs> <hex ptau> <cuts|->      the r1cs is cut (the ptau whole)
//   setupp <hex r1cs> <hex ptau> <cuts|->     the ptau is cut (the r1cs whole)
//   contribute <hex zkey> <hex secret, 32 B LE> <cuts|->
//   vk <hex zkey> - <cuts|->
// cuts: comma-separated lengths; the input is opened once per cut from a heap block of exactly
// that many bytes ("-": its whole length), so a read past the end is a sanitizer report. Per
// block: "ERR <code>" or "OK <hex of the result>" (vk: the JSON text as it is).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nzcb-circom_amd/csrc/groth16.h"

using namespace nzcb;

static std::vector<uint8_t> unhex(const std::string& hex) {
  std::vector<uint8_t> b(hex.size() / 2);
  for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
  return b;
}

static std::string hex_of(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

struct Block {  // exactly the bytes: no slack to read into
  uint8_t* p;
  size_t len;
  Block(const std::vector<uint8_t>& v, size_t n) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))), len(n) {
    std::memcpy(p, v.data(), n);
  }
  ~Block() { std::free(p); }
};

template <class Fn>
static void answer(Fn fn) {
  try {
    fn();
  } catch (const Error& e) {
    std::printf("ERR %d\n", e.code);
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, a, b, c;
    in >> kind >> a >> b >> c;
    const std::vector<uint8_t> first = unhex(a), second = b == "-" ? std::vector<uint8_t>() : unhex(b);
    const std::vector<uint8_t>& cut_in = kind == "setupp" ? second : first;
    std::vector<size_t> lens;
    if (c == "-" || c.empty()) {
      lens.push_back(cut_in.size());
    } else {
      std::istringstream cs(c);
      std::string cut;
      while (std::getline(cs, cut, ',')) lens.push_back(std::min(cut_in.size(), (size_t)std::stoull(cut)));
    }
    for (size_t len : lens) {
      const Block blk(cut_in, len);
      answer([&] {
        if (kind == "setup" || kind == "setupp") {
          G16HostBackend be;
          PtauOut o;
          if (kind == "setup")
            g16_setup(be, blk.p, blk.len, second.data(), second.size(), nullptr, o);
          else
            g16_setup(be, first.data(), first.size(), blk.p, blk.len, nullptr, o);
          std::printf("OK %s\n", hex_of(o.p, (size_t)o.len).c_str());
        } else if (kind == "contribute") {
          G16HostBackend be;
          PtauOut o;
          Fr d;
          make_secrets(second.size() == 32 ? second.data() : nullptr, nullptr, 0, &d, 1, "zkey");
          g16_contribute(be, blk.p, blk.len, d, nullptr, o);
          std::printf("OK %s\n", hex_of(o.p, (size_t)o.len).c_str());
        } else {
          std::printf("OK %s\n", g16_vk_json(blk.p, blk.len).c_str());
        }
      });
    }
  }
  return 0;
}
