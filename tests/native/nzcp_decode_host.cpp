// csrc/nzcp_decode.h built for the host under AddressSanitizer and UBSan (tests/
// test_nzcp_decode_native.py): the bounds check of the shared decoder source. Reads one URI per
// line from stdin as hex ("-" is the empty URI), copies it into a heap allocation of exactly its
// length, so that a read past either end is caught, decodes it for the live circuit with the data
// bytes 1..20, and prints the record as hex, then the SHA-256 of the pass's input block.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nzcb-circom_amd/csrc/nzcp_decode.h"

using namespace nzcb::nzdec;

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

static void put_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) std::printf("%02x", p[i]);
}

int main() {
  const uint32_t max_tbs = 351;
  const size_t block = (size_t)input_signals(max_tbs) * 32;
  std::string line;
  int ch;
  auto run = [&] {
    const size_t len = line == "-" ? 0 : line.size() / 2;
    uint8_t* uri = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len == 0) {  // an allocation of no bytes at all: any read is out of bounds
      std::free(uri);
      uri = static_cast<uint8_t*>(std::malloc(0));
    }
    for (size_t i = 0; i < len; i++) {
      const int hi = nibble(line[2 * i]), lo = nibble(line[2 * i + 1]);
      if (hi < 0 || lo < 0) std::exit(2);
      uri[i] = (uint8_t)(hi << 4 | lo);
    }
    uint8_t* data = static_cast<uint8_t*>(std::malloc(kDataBytes));
    for (uint32_t i = 0; i < kDataBytes; i++) data[i] = (uint8_t)(i + 1);
    uint8_t* cose = static_cast<uint8_t*>(std::malloc(kMaxCose));
    uint8_t* tbs = static_cast<uint8_t*>(std::malloc(kMaxTbs));
    uint8_t* inputs = static_cast<uint8_t*>(std::malloc(block));
    uint8_t* tbs_out = static_cast<uint8_t*>(std::malloc(max_tbs));
    nzcb_nzcp_pass* rec = static_cast<nzcb_nzcp_pass*>(std::malloc(sizeof(nzcb_nzcp_pass)));
    decode_one(uri, len, max_tbs, data, cose, tbs, rec, inputs, tbs_out, max_tbs);
    uint8_t digest[32];
    sha256(inputs, (uint32_t)block, digest);
    put_hex(reinterpret_cast<const uint8_t*>(rec), sizeof(*rec));
    std::printf(" ");
    put_hex(digest, 32);
    std::printf("\n");
    for (void* p : {(void*)uri, (void*)data, (void*)cose, (void*)tbs, (void*)inputs, (void*)tbs_out, (void*)rec})
      std::free(p);
  };
  while ((ch = std::getchar()) != EOF) {
    if (ch == '\n') {
      if (!line.empty()) run();
      line.clear();
    } else {
      line.push_back((char)ch);
    }
  }
  if (!line.empty()) run();
  return 0;
}
