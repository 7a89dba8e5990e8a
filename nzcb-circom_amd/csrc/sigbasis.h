// The signal basis of a PLONK proving key: A, B and C committed over the witness signals
// instead of the gate slots (DESIGN.md §4 "A, B, C").
//
// The gate values are linear in the witness and the map is fixed by the key: gate g's A wire
// holds a variable, which is a witness signal or an addition dst = ac a + bc b over earlier
// variables. With coefA(g, s) the coefficient of signal s in that variable once the additions
// are expanded,
//   [A] = sum_{s < nWit} w_s SA_s + b_lo ([tau^n] - [1]) + b_hi ([tau^(n+1)] - [tau]),
//   SA_s = sum_g coefA(g, s) [L_g(tau)],
// the same group element as the commitment over the n + 2 Lagrange points, from nWit scalars
// instead of n. SA_s is a Groth16 A-query row: the rows are computed once per context by the
// Groth16 row kernels (groth16.h G16RowsBuilder, g16_plan; groth16.hip) over the device-resident
// Lagrange basis.
//
// Each set (A, B, C) is compacted to the signals that have a row in it; the three sets are laid
// into one base array of 3 x stride points: the set's rows, then its two blinding points, then
// points at infinity up to stride (their scalars are staged as zero, so they make no entry).
#pragma once
#include <string>
#include <vector>

#include "ec.h"

namespace nzcb {

struct SigBasis {
  bool ok = false;
  std::string note;              // why not, when !ok (one log line)
  uint32_t cnt[3] = {0, 0, 0};   // rows per set
  size_t stride = 0;             // max(cnt) + 2
  std::vector<uint32_t> idx;     // 3 x stride: the signal of each row (kSigNone past the rows)
  std::vector<G1Affine> bases;   // 3 x stride, LEM affine
  uint64_t terms = 0;            // (set, signal, gate) terms after the expansion
  uint64_t expanded = 0;         // terms held by the additions' own expansions
};
constexpr uint32_t kSigNone = 0xffffffffu;
constexpr uint64_t kSigCapDefault = 64;

// The expansion gives up (SigBasis::ok = false, the context commits from the Lagrange basis) once
// it holds more than cap * 3 * nConstraints terms: snarkjs folds linear combinations by halving,
// so honest keys stay far below, but a key may chain its additions. Set for the contexts created
// after the call (nzcb_debug_signal_basis_cap); returns the previous value.
uint64_t sig_basis_cap(int64_t per_constraint = -2);

// d_ltau: the context's n + 2 Lagrange-basis points on `device` (complete: the caller has
// synchronised the stream that built them). additions: nAdditions x 72 bytes (zkey section 3);
// the maps: nConstraints variable indices each (host). max_stride: the largest stride the
// context's MSM scratch takes.
SigBasis sig_basis_build(int device, const G1Affine* d_ltau, uint32_t n, uint32_t nWit, uint32_t nVars,
                         uint32_t nConstraints, const uint8_t* additions, uint32_t nAdditions,
                         const uint8_t* amap, const uint8_t* bmap, const uint8_t* cmap, size_t max_stride);

}  // namespace nzcb
