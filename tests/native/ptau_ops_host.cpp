// Stand-alone host build of csrc/ptau_ops.h for tests/test_ptau_ops_native.py: the section
// reader and writer of the powers-of-tau operations, the point tests and the point arithmetic
// over Fq and Fq2, compiled with -fsanitize=address,undefined. stdin, one request per line:
//   ptau <hex of the file> <cut,cut,...|->   the file is opened once per cut from a heap block of
//        exactly `cut` bytes ("-": its whole length), so a read past the end is a sanitizer
//        report. Per block: "ERR <code>" or "OK <power> <one status digit per point of section 2>
//        <section 3> <4> <5> <6>"
//   new <power>                              "ERR <code>" or "OK <hex of nzcb_ptau_new's bytes>"
//   mul <g1|g2> <hex of the point> <hex of the scalar, 32 B LE>   "OK <hex of scalar * point>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nzcb-circom_amd/csrc/ptau_ops.h"

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

template <class F>
static std::string digits(const PtauSections& f, int id, const Fq2& b2) {
  std::string s;
  for (uint64_t i = 0; i < f.points(id); i++) {
    PtAffine<F> p;
    std::memcpy((void*)&p, f.s[id].p + sizeof p * i, sizeof p);
    s += (char)('0' + pt_status<F>(&p, b2));
  }
  return s;
}

static void examine(const uint8_t* d, size_t len) {
  try {
    const PtauSections f = ptau_sections_open(d, len);
    const Fq2 b2 = g2_twist_b();
    std::printf("OK %u %s %s %s %s %s\n", f.power, digits<Fq>(f, 2, b2).c_str(), digits<Fq2>(f, 3, b2).c_str(),
                digits<Fq>(f, 4, b2).c_str(), digits<Fq>(f, 5, b2).c_str(), digits<Fq2>(f, 6, b2).c_str());
  } catch (const Error& e) {
    std::printf("ERR %d\n", e.code);
  }
}

template <class F>
static void mul(const std::vector<uint8_t>& pt, const std::vector<uint8_t>& k) {
  PtAffine<F> p;
  Fr s;
  if (pt.size() != sizeof p || k.size() != sizeof s) {
    std::printf("ERR %d\n", NZCB_ERR_ARG);
    return;
  }
  std::memcpy((void*)&p, pt.data(), sizeof p);
  std::memcpy(s.v, k.data(), sizeof s);
  const PtAffine<F> r = pt_to_affine(pt_mul_affine(p, s));
  // the same through the general addition and the scalar a contribution derives
  const PtAffine<F> r2 = pt_to_affine(pt_mul(pt_from_affine(p), ptau_scalar(to_mont(s), Fr::one(), 7)));
  if (std::memcmp(&r, &r2, sizeof r) != 0) {
    std::printf("ERR %d\n", NZCB_ERR_INTERNAL);
    return;
  }
  std::printf("OK %s\n", hex_of(reinterpret_cast<const uint8_t*>(&r), sizeof r).c_str());
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, a, b, c;
    in >> kind >> a >> b >> c;
    if (kind == "new") {
      try {
        PtauOut o;
        ptau_new(std::stoi(a), o, nullptr);
        std::printf("OK %s\n", hex_of(o.p, (size_t)o.len).c_str());
      } catch (const Error& e) {
        std::printf("ERR %d\n", e.code);
      }
    } else if (kind == "mul") {
      if (a == "g2")
        mul<Fq2>(unhex(b), unhex(c));
      else
        mul<Fq>(unhex(b), unhex(c));
    } else {
      const std::vector<uint8_t> file = unhex(a);
      std::vector<size_t> lens;
      if (b == "-") {
        lens.push_back(file.size());
      } else {
        std::istringstream cs(b);
        std::string cut;
        while (std::getline(cs, cut, ',')) lens.push_back(std::min(file.size(), (size_t)std::stoull(cut)));
      }
      for (size_t len : lens) {
        uint8_t* block = static_cast<uint8_t*>(std::malloc(len ? len : 1));  // exactly the file: no slack to read into
        std::memcpy(block, file.data(), len);
        examine(block, len);
        std::free(block);
      }
    }
  }
  return 0;
}
