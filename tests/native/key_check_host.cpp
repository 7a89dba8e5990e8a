// Stand-alone host build of csrc/key_check.h for tests/test_key_check_native.py: the section
// walker, the ptau reader and the per-point and per-value judgements, compiled with
// -fsanitize=address,undefined. stdin: one line per file, "<ptau|zkey> <hex of the file>
// <cut,cut,...|->"; the file is examined once per cut from a heap block of exactly `cut` bytes
// ("-": its whole length), so a read past the end is a sanitizer report. stdout, per block:
//   ptau: "ERR <code>" or "OK <power> <one status digit per tauG1 point>"
//   zkey: "ERR <code>" or "OK <one status digit per section-14 point> <values >= r in sections 7..13>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nzcb-circom_amd/csrc/key_check.h"

using namespace nzcb;

static std::string point_digits(const uint8_t* p, uint64_t count) {
  std::string s;
  for (uint64_t i = 0; i < count; i++) {
    uint32_t w[16];
    std::memcpy(w, p + 64 * i, 64);
    s += (char)('0' + srs_point_status(w));
  }
  return s.empty() ? "-" : s;
}

static void examine(const std::string& kind, const uint8_t* d, size_t len) {
  try {
    if (kind == "ptau") {
      const PtauView v = ptau_open(d, len, 0);
      std::printf("OK %u %s\n", v.power, point_digits(v.g1, v.count).c_str());
      return;
    }
    const KeySection pts = key_find_section(d, len, "zkey", 14);
    uint64_t noncanonical = 0;
    for (uint32_t id = 7; id <= 13; id++) {
      const KeySection s = key_find_section(d, len, "zkey", id);
      for (uint64_t i = 0; i + 32 <= s.len; i += 32) {
        uint32_t w[8];
        std::memcpy(w, s.p + i, 32);
        noncanonical += fr_noncanonical(w) ? 1 : 0;
      }
    }
    std::printf("OK %s %llu\n", point_digits(pts.p, pts.len / 64).c_str(), (unsigned long long)noncanonical);
  } catch (const Error& e) {
    std::printf("ERR %d\n", e.code);
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, hex, cuts;
    in >> kind >> hex >> cuts;
    std::vector<uint8_t> file(hex.size() / 2);
    for (size_t i = 0; i < file.size(); i++) file[i] = (uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
    std::vector<size_t> lens;
    if (cuts == "-") {
      lens.push_back(file.size());
    } else {
      std::istringstream cs(cuts);
      std::string c;
      while (std::getline(cs, c, ',')) lens.push_back(std::min(file.size(), (size_t)std::stoull(c)));
    }
    for (size_t len : lens) {
      uint8_t* block = static_cast<uint8_t*>(std::malloc(len ? len : 1));  // exactly the file: no slack to read into
      std::memcpy(block, file.data(), len);
      examine(kind, block, len);
      std::free(block);
    }
  }
  return 0;
}
