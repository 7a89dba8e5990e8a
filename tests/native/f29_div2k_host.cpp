// Host build of csrc/f29.h's div2k29 (NZ_HD = inline without HIP): reads "<K> <9 hex limbs>"
// lines on stdin and prints the 9 hex limbs of div2k29(x, K), which tests/test_f29_div2k.py
// compares with exact integers.
#include <cstdio>

#include "../../nzcb-circom_amd/csrc/f29.h"

using namespace nzcb;

int main() {
  int k;
  while (std::scanf("%d", &k) == 1) {
    if (k < 1 || k > 28) return 2;
    F29 x;
    for (int i = 0; i < 9; i++)
      if (std::scanf("%x", &x.v[i]) != 1) return 3;
    const F29 r = div2k29(x, k);
    for (int i = 0; i < 9; i++) std::printf("%x%c", r.v[i], i == 8 ? '\n' : ' ');
  }
  return 0;
}
