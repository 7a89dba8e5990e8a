// The signal basis (sigbasis.h): the additions expanded on the host, the rows by the Groth16 row
// kernels (groth16.hip) over the context's Lagrange basis, compacted per set.
#include "sigbasis.h"

#include <atomic>
#include <cstring>

#include "groth16.h"

namespace nzcb {

static std::atomic<uint64_t> g_sig_cap{kSigCapDefault};

uint64_t sig_basis_cap(int64_t per_constraint) {
  if (per_constraint == -2) return g_sig_cap.load();
  return g_sig_cap.exchange(per_constraint < 0 ? kSigCapDefault : (uint64_t)per_constraint);
}

namespace {

struct SigTerm {
  uint32_t s;
  Fr c;  // Montgomery
};

}  // namespace

SigBasis sig_basis_build(int device, const G1Affine* d_ltau, uint32_t n, uint32_t nWit, uint32_t nVars,
                         uint32_t nConstraints, const uint8_t* additions, uint32_t nAdditions,
                         const uint8_t* amap, const uint8_t* bmap, const uint8_t* cmap, size_t max_stride) {
  SigBasis sb;
  const uint64_t cap = sig_basis_cap() * 3 * (uint64_t)nConstraints;
  auto give_up = [&](const std::string& why) {
    sb.ok = false;
    sb.note = "signal basis: " + why + "; A, B, C are committed from the Lagrange basis";
    return sb;
  };
  // the additions' expansions over the witness signals, each sorted by signal. Variable 0 reads
  // as zero (k_wit_to_mont), references past nVars and forward references read as zero
  // (k_additions' kZeroRef), and a coefficient that cancels is no term.
  std::vector<uint64_t> off((size_t)nAdditions + 1, 0);
  std::vector<SigTerm> ex;
  std::vector<SigTerm> ta, tb;
  for (uint32_t k = 0; k < nAdditions; k++) {
    const uint8_t* p = additions + (size_t)k * 72;
    uint32_t ai, bi;
    Fr ac, bc;
    std::memcpy(&ai, p, 4);
    std::memcpy(&bi, p + 4, 4);
    std::memcpy(ac.v, p + 8, 32);
    std::memcpy(bc.v, p + 40, 32);
    auto operand = [&](uint32_t v, const Fr& coef, std::vector<SigTerm>& out) {
      out.clear();
      if (v == 0 || v >= nVars) return;
      if (v < nWit) {
        out.push_back({v, coef});
        return;
      }
      const uint32_t kk = v - nWit;
      if (kk >= k) return;
      for (uint64_t t = off[kk]; t < off[kk + 1]; t++) out.push_back({ex[t].s, coef * ex[t].c});
    };
    operand(ai, ac, ta);
    operand(bi, bc, tb);
    size_t i = 0, j = 0;
    auto put = [&](uint32_t s, const Fr& c) {
      if (!reduce_once(c).is_zero()) ex.push_back({s, c});
    };
    while (i < ta.size() || j < tb.size()) {
      if (j == tb.size() || (i < ta.size() && ta[i].s < tb[j].s)) {
        put(ta[i].s, ta[i].c);
        i++;
      } else if (i == ta.size() || tb[j].s < ta[i].s) {
        put(tb[j].s, tb[j].c);
        j++;
      } else {
        put(ta[i].s, ta[i].c + tb[j].c);
        i++;
        j++;
      }
    }
    off[k + 1] = ex.size();
    if (ex.size() > cap) return give_up("the additions expand past " + std::to_string(cap) + " terms");
  }
  sb.expanded = ex.size();

  // rows (set, signal) over the points [L_g(tau)], g < n; a gate's wire holds one variable, whose
  // expansion names a signal once, so (set, signal, gate) is one term
  const uint32_t gates = nConstraints < n ? nConstraints : n;
  G16RowsBuilder b((uint64_t)3 * nWit, n);
  const uint8_t* maps[3] = {amap, bmap, cmap};
  for (int set = 0; set < 3; set++) {
    for (uint32_t g = 0; g < gates; g++) {
      uint32_t v;
      std::memcpy(&v, maps[set] + (size_t)g * 4, 4);
      if (v == 0 || v >= nVars) continue;
      if (v < nWit) {
        b.add((uint64_t)set * nWit + v, g, Fr::one());
        sb.terms++;
      } else {
        const uint32_t kk = v - nWit;
        for (uint64_t t = off[kk]; t < off[kk + 1]; t++) b.add((uint64_t)set * nWit + ex[t].s, g, ex[t].c);
        sb.terms += off[kk + 1] - off[kk];
      }
      if (sb.terms > cap) return give_up("the gates expand past " + std::to_string(cap) + " terms");
    }
  }
  ex.clear();
  ex.shrink_to_fit();
  G16Rows rows = b.finish();
  const G16Schedule sch = g16_schedule();
  const G16Plan plan = g16_plan(rows, sch.chunk, sch.fan_in);
  std::vector<G1Affine> out((size_t)3 * nWit);
  g16_rows_g1_device(device, reinterpret_cast<const G1Pt*>(d_ltau), rows, plan, reinterpret_cast<uint8_t*>(out.data()));

  // a row that has terms and is not the point at infinity (which commits nothing) is present
  auto present = [&](size_t r) { return rows.row_off[r + 1] > rows.row_off[r] && !out[r].is_inf(); };
  uint32_t most = 0;
  for (int set = 0; set < 3; set++) {
    for (uint32_t s = 0; s < nWit; s++) sb.cnt[set] += present((size_t)set * nWit + s) ? 1u : 0u;
    most = sb.cnt[set] > most ? sb.cnt[set] : most;
  }
  sb.stride = (size_t)most + 2;
  if (sb.stride > max_stride)
    return give_up("a set has " + std::to_string(most) + " signals, more than the " + std::to_string(n) + " gate slots");
  G1Affine tail[2];
  if (hipMemcpy(tail, d_ltau + n, sizeof tail, hipMemcpyDeviceToHost) != hipSuccess)
    throw Error(NZCB_ERR_HIP, "signal basis: reading the blinding points failed");
  G1Affine inf;
  inf.x = Fq::zero();
  inf.y = Fq::zero();
  sb.idx.assign(3 * sb.stride, kSigNone);
  sb.bases.assign(3 * sb.stride, inf);
  for (int set = 0; set < 3; set++) {
    size_t at = (size_t)set * sb.stride;
    for (uint32_t s = 0; s < nWit; s++) {
      const size_t r = (size_t)set * nWit + s;
      if (!present(r)) continue;
      sb.idx[at] = s;
      sb.bases[at++] = out[r];
    }
    sb.bases[at] = tail[0];
    sb.bases[at + 1] = tail[1];
  }
  sb.ok = true;
  return sb;
}

}  // namespace nzcb
