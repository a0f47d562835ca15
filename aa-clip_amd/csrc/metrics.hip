// Device metrics_eval (reference forward_utils.py:233-280): the
// class-global min-max normalisation of the pixel maps and image scores, the
// pixel-max fusion of the image score, and EXACT sklearn roc_auc_score /
// average_precision_score (tie-aware) for pixels and images.
//
// Pixels (up to ~19 M per class at C4) are ranked by one radix sort of 33-bit
// keys: (order-preserving bits of the normalised fp32 score << 1) | label, so
// equal scores form contiguous groups with their negatives first. Then
//   * AUROC = U / (P*N), U the Mann-Whitney count (pairs pos > neg, ties 1/2),
//     equal to sklearn's trapezoid over the tie-grouped ROC curve; 2U is summed
//     exactly in 64-bit integers;
//   * AP = (1/P) * sum over positives of TP(>= s) / N(>= s), i.e. sklearn's
//     sum_n (R_n - R_{n-1}) P_n over distinct thresholds, in fp64.
// Per sorted position i both need only P_excl[i] (positives before i: a scan of
// the label bits) and a_g (start of i's score group: a max-scan of flagged
// indices). Reductions are two-level and fixed-order, so results are
// deterministic run to run. Images (hundreds) use direct O(n^2) pair counts.
// Sort and scans are rocPRIM device primitives; the caller owns all memory
// (workspace size from aaclip_metrics_workspace).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "scorenorm.h"

namespace {

// One block: global min/max, normalisation flags, fused image scores.
__global__ __launch_bounds__(MT) void image_scores_kernel(const float* __restrict__ rmin,
                                                          const float* __restrict__ rmax,
                                                          const float* __restrict__ img, int n_img, int medical,
                                                          Norm* __restrict__ nrm, float* __restrict__ fused) {
  __shared__ float sh[MT / 64];
  float lo = INFINITY, hi = -INFINITY, ilo = INFINITY, ihi = -INFINITY;
  for (int i = threadIdx.x; i < n_img; i += MT) {
    lo = fminf(lo, rmin[i]);
    hi = fmaxf(hi, rmax[i]);
    ilo = fminf(ilo, img[i]);
    ihi = fmaxf(ihi, img[i]);
  }
  lo = block_min(lo, sh);
  hi = block_max(hi, sh);
  ilo = block_min(ilo, sh);
  ihi = block_max(ihi, sh);
  const bool pn = norm_wanted(hi), in = norm_wanted(ihi);
  if (threadIdx.x == 0) *nrm = Norm{lo, hi, ilo, ihi, pn, in};
  for (int i = threadIdx.x; i < n_img; i += MT) {
    // max over pixels of the normalised map == normalised row max: fl((x-a)/b) is monotone
    const float pm = pn ? norm_apply(rmax[i], lo, hi) : rmax[i];
    const float is = in ? norm_apply(img[i], ilo, ihi) : img[i];
    fused[i] = medical ? pm : pm * 0.5f + is * 0.5f;
  }
}

__global__ __launch_bounds__(MT) void make_keys_kernel(const float* __restrict__ p, const uint8_t* __restrict__ lab,
                                                       int64_t n, const Norm* __restrict__ nrm,
                                                       uint64_t* __restrict__ keys) {
  const Norm z = *nrm;
  for (int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT) {
    const float v = pixel_score(p[i], z);
    keys[i] = ((uint64_t)ord_bits(v) << 1) | (lab[i] != 0 ? 1u : 0u);
  }
}

// label bit and flagged group-start index of every sorted position
__global__ __launch_bounds__(MT) void split_keys_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                        uint32_t* __restrict__ lbl, uint32_t* __restrict__ gstart) {
  for (int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT) {
    const uint64_t k = keys[i];
    lbl[i] = (uint32_t)(k & 1);
    gstart[i] = (i == 0 || (keys[i - 1] >> 1) != (k >> 1)) ? (uint32_t)i : 0u;
  }
}

struct Partial {
  unsigned long long u2;  // 2U contribution
  double ap;              // sum of TP(>=s)/N(>=s) over positives
};

__device__ __forceinline__ Partial block_sum(Partial v, Partial* sh) {
  for (int o = 32; o > 0; o >>= 1) {
    v.u2 += __shfl_xor(v.u2, o, 64);
    v.ap += __shfl_xor(v.ap, o, 64);
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  Partial r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
    r.u2 += sh[i].u2;
    r.ap += sh[i].ap;
  }
  return r;
}

// pixel pass over sorted positions: P = exclusive label scan (P[n] = total),
// A = inclusive max-scan of group starts. Deterministic per-block partials.
__global__ __launch_bounds__(MT) void pixel_partial_kernel(const uint32_t* __restrict__ lbl,
                                                           const uint32_t* __restrict__ P,
                                                           const uint32_t* __restrict__ A, int64_t n,
                                                           int64_t per_block, Partial* __restrict__ part) {
  __shared__ Partial sh[MT / 64];
  const uint64_t ptot = (uint64_t)P[n - 1] + lbl[n - 1];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = min(n, lo + per_block);
  Partial acc{0ull, 0.0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += MT) {
    if (!lbl[i]) continue;
    const uint64_t a = A[i];
    const uint64_t pa = P[a];
    const uint64_t nb_i = (uint64_t)i - P[i];  // negatives at positions < i (incl. this group's)
    const uint64_t nb_a = a - pa;              // negatives strictly below the group
    acc.u2 += nb_i + nb_a;
    acc.ap += (double)(ptot - pa) / (double)((uint64_t)n - a);
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// image pass: O(n^2) pair counts, one thread per image
__global__ __launch_bounds__(MT) void image_partial_kernel(const float* __restrict__ s,
                                                           const uint8_t* __restrict__ lab, int n,
                                                           Partial* __restrict__ part) {
  __shared__ Partial sh[MT / 64];
  Partial acc{0ull, 0.0};
  const int i = blockIdx.x * MT + threadIdx.x;
  if (i < n && lab[i]) {
    const float si = s[i];
    uint64_t below = 0, eq_neg = 0, ge = 0, ge_pos = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s[j];
      const bool pj = lab[j] != 0;
      if (sj >= si) {
        ++ge;
        ge_pos += pj;
      }
      if (!pj) {
        below += sj < si;
        eq_neg += sj == si;
      }
    }
    acc.u2 = 2 * below + eq_neg;
    acc.ap = (double)ge_pos / (double)ge;
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// out[0..1] = pixel AUROC, AP; out[2..3] = image AUROC, AP (0, 0 when the image
// labels are all equal, forward_utils.py:264-271; NaN when the pixel labels are,
// where sklearn raises).
__global__ __launch_bounds__(64) void finalize_kernel(const Partial* __restrict__ pp, int npp,
                                                     const uint32_t* __restrict__ P,
                                                     const uint32_t* __restrict__ lbl, int64_t n,
                                                     const Partial* __restrict__ ip, int nip,
                                                     const uint8_t* __restrict__ ilab, int n_img,
                                                     double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  Partial a{0ull, 0.0};
  for (int i = 0; i < npp; ++i) {
    a.u2 += pp[i].u2;
    a.ap += pp[i].ap;
  }
  const uint64_t pos = (uint64_t)P[n - 1] + lbl[n - 1], neg = (uint64_t)n - pos;
  if (pos == 0 || neg == 0) {
    out[0] = out[1] = NAN;
  } else {
    out[0] = (double)a.u2 / (2.0 * (double)pos * (double)neg);
    out[1] = a.ap / (double)pos;
  }
  Partial b{0ull, 0.0};
  for (int i = 0; i < nip; ++i) {
    b.u2 += ip[i].u2;
    b.ap += ip[i].ap;
  }
  uint64_t ipos = 0;
  for (int i = 0; i < n_img; ++i) ipos += ilab[i] != 0;
  const uint64_t ineg = (uint64_t)n_img - ipos;
  if (ipos == 0 || ineg == 0) {
    out[2] = out[3] = 0.0;
  } else {
    out[2] = (double)b.u2 / (2.0 * (double)ipos * (double)ineg);
    out[3] = b.ap / (double)ipos;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Pixel AUPRO (aaclip_metrics_eval_pro): the area under the per-region-overlap curve up to a
// false-positive rate L, over the same sorted pixels. Regions are the 8-connected components of
// the masks (aaclip_label_components); every positive pixel carries its component's area through
// the sort as the 32-bit value of radix_sort_pairs on the same 33-bit keys, so the sorted keys,
// and with them out[0..3], are those of aaclip_metrics_eval bit for bit.
//
// Per positive pixel i of a component of area |r| (R components, N_ok negatives), with A_i the
// negatives scored strictly above s_i and B_i = A_i + the negatives tied with s_i, the pixel's
// share of PRO rises linearly from 0 to 1 / (|r| R) while FPR goes from A_i / N_ok to B_i / N_ok.
// Its area under the curve up to L, times N_ok |r| R, with K = L N_ok:
//   0                          if A_i >= K
//   (B_i - A_i) / 2 + K - B_i  if B_i <= K
//   (K - A_i)^2 / (2 (B_i - A_i))  otherwise
// A_i and B_i are integers from P (exclusive label scan) and the group start a: the group's
// negatives sort first (the label is the key's low bit), so B_i = (n - a) - (P_total - P[a]) and
// the group holds (i - a) - (P[i] - P[a]) negatives. The sum is fp64, two-level, fixed order.
namespace {

struct ProTotals {
  unsigned long long regions;  // R over the class
  unsigned int failed;         // a labelling loop hit its cap (never, unless there is a bug)
  unsigned int pad;
};

__global__ __launch_bounds__(64) void pro_totals_kernel(const uint32_t* __restrict__ counts, int n_img,
                                                       ProTotals* __restrict__ tot) {
  if (threadIdx.x != 0) return;
  ProTotals t{0ull, 0u, 0u};
  for (int i = 0; i < n_img; ++i) {
    t.regions += counts[i];
    t.failed |= counts[i] == 0xFFFFFFFFu;
  }
  *tot = t;
}

__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  double r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
  return r;
}

// the layout of pixel_partial_kernel: block b sums sorted positions [b * per_block, (b + 1) * per_block)
__global__ __launch_bounds__(MT) void pro_partial_kernel(const uint32_t* __restrict__ lbl,
                                                         const uint32_t* __restrict__ P,
                                                         const uint32_t* __restrict__ A,
                                                         const uint32_t* __restrict__ area, int64_t n,
                                                         int64_t per_block, double fpr_limit,
                                                         double* __restrict__ part) {
  __shared__ double sh[MT / 64];
  const uint64_t ptot = (uint64_t)P[n - 1] + lbl[n - 1];
  const double K = fpr_limit * (double)((uint64_t)n - ptot);
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = min(n, lo + per_block);
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += MT) {
    if (!lbl[i]) continue;
    const uint64_t a = A[i];
    const uint64_t pa = P[a];
    const uint64_t tied = ((uint64_t)i - a) - (P[i] - pa);   // this group's negatives
    const uint64_t ge = ((uint64_t)n - a) - (ptot - pa);     // negatives scored >= s_i
    const double B = (double)ge, Ab = (double)(ge - tied), w = (double)tied;
    double c;
    if (Ab >= K) c = 0.0;
    else if (B <= K) c = 0.5 * w + (K - B);
    else c = (K - Ab) * (K - Ab) / (2.0 * w);
    acc += c / (double)area[i];
  }
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// out[4] = AUPRO; NaN with no region or no negative pixel (where the pixel AUROC is NaN too)
__global__ __launch_bounds__(64) void pro_finalize_kernel(const double* __restrict__ part, int npp,
                                                         const uint32_t* __restrict__ P,
                                                         const uint32_t* __restrict__ lbl, int64_t n,
                                                         const ProTotals* __restrict__ tot, double fpr_limit,
                                                         double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < npp; ++i) s += part[i];
  const uint64_t pos = (uint64_t)P[n - 1] + lbl[n - 1], neg = (uint64_t)n - pos;
  const ProTotals t = *tot;
  if (t.failed || t.regions == 0 || neg == 0)
    out[4] = NAN;
  else
    out[4] = s / ((double)t.regions * (double)neg * fpr_limit);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// F1-max and its threshold (aaclip_metrics_eval_f1), pixels and images, from what the passes above
// leave behind: the sorted keys, the exclusive label scan P and the group starts A. With v the
// class-normalised fp32 score, P_tot the positives and n the count, every distinct score t has
//   PP(t) = #{v >= t},  TP(t) = #{y = 1, v >= t},  F1(t) = (double)(2 TP) / (double)(PP + P_tot):
// two exact integers and one fp64 division, so a float64 restatement gets the same bits. On the
// ascending sorted array the candidates are the group starts a (A[a] == a): PP = n - a,
// TP = P_tot - P[a]. The maximum is taken with ties to the lower position, i.e. the lowest
// threshold, per thread (ascending, strict >), per wave and block (total order on (F1, position)),
// then over the block partials in order: no atomics, the same bits whatever the grid.
namespace {

struct F1Best {
  double f1;               // -1 when the block has no group start
  unsigned long long pos;  // the group start's sorted position
};

__device__ __forceinline__ bool f1_before(const F1Best& a, const F1Best& b) {
  return a.f1 > b.f1 || (a.f1 == b.f1 && a.pos < b.pos);
}

// the layout of pixel_partial_kernel: block b looks at sorted positions [b * per_block, (b + 1) * per_block)
__global__ __launch_bounds__(MT) void f1_partial_kernel(const uint32_t* __restrict__ lbl,
                                                        const uint32_t* __restrict__ P,
                                                        const uint32_t* __restrict__ A, int64_t n,
                                                        int64_t per_block, F1Best* __restrict__ part) {
  __shared__ F1Best sh[MT / 64];
  const uint64_t ptot = (uint64_t)P[n - 1] + lbl[n - 1];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = min(n, lo + per_block);
  F1Best best{-1.0, ~0ull};
  constexpr int U = 8;  // loads in flight per thread; positions are still visited in ascending order
  for (int64_t base = lo + threadIdx.x; base < hi; base += (int64_t)U * MT) {
    uint32_t a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * MT;
      a[u] = i < hi ? A[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + (int64_t)u * MT;
      if (i >= hi || a[u] != (uint32_t)i) continue;  // past the end, or not a group start
      const uint64_t tp = ptot - P[i], pp = (uint64_t)n - (uint64_t)i;
      const double f = (double)(2 * tp) / (double)(pp + ptot);
      if (f > best.f1) best = F1Best{f, (unsigned long long)i};
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const F1Best other{__shfl_xor(best.f1, o, 64), __shfl_xor(best.pos, o, 64)};
    if (f1_before(other, best)) best = other;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh[w] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    F1Best r = sh[0];
    for (int i = 1; i < MT / 64; ++i)
      if (f1_before(sh[i], r)) r = sh[i];
    part[blockIdx.x] = r;
  }
}

struct F1Image {
  double f1;     // -1 for a thread without an image
  uint32_t key;  // ord_bits of the candidate score
  uint32_t tp, pp;
  uint32_t pad;
};

// equal scores give equal counts, so (F1, score) orders every distinct record
__device__ __forceinline__ bool f1_before(const F1Image& a, const F1Image& b) {
  return a.f1 > b.f1 || (a.f1 == b.f1 && a.key < b.key);
}

// image pass: one thread per candidate threshold s[i], O(n^2) counts. Scores are compared as
// the pixel keys are (ord_bits), so that, as there, a score that normalised to 0 / 0 is one tie group.
__global__ __launch_bounds__(MT) void f1_image_partial_kernel(const float* __restrict__ s,
                                                              const uint8_t* __restrict__ lab, int n,
                                                              F1Image* __restrict__ part) {
  __shared__ F1Image sh[MT / 64];
  F1Image best{-1.0, 0u, 0u, 0u, 0u};
  const int i = blockIdx.x * MT + threadIdx.x;
  if (i < n) {
    const uint32_t ki = ord_bits(s[i]);
    uint32_t pos = 0, ge = 0, ge_pos = 0;
    for (int j = 0; j < n; ++j) {
      const bool pj = lab[j] != 0;
      pos += pj;
      if (ord_bits(s[j]) >= ki) {
        ++ge;
        ge_pos += pj;
      }
    }
    best = F1Image{(double)(2 * (uint64_t)ge_pos) / (double)((uint64_t)ge + pos), ki, ge_pos, ge, 0u};
  }
  for (int o = 32; o > 0; o >>= 1) {
    const F1Image other{__shfl_xor(best.f1, o, 64), __shfl_xor(best.key, o, 64), __shfl_xor(best.tp, o, 64),
                        __shfl_xor(best.pp, o, 64), 0u};
    if (f1_before(other, best)) best = other;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh[w] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    F1Image r = sh[0];
    for (int k = 1; k < MT / 64; ++k)
      if (f1_before(sh[k], r)) r = sh[k];
    part[blockIdx.x] = r;
  }
}

// out[5..8] = pixel F1-max, threshold, precision, recall (NaN where the pixel AUROC is NaN);
// out[9..12] = the same for images (0 when the image labels are all equal, as out[2..3]);
// out[4] = NaN when no AUPRO was computed
__global__ __launch_bounds__(64) void f1_finalize_kernel(const F1Best* __restrict__ pp, int npp,
                                                        const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ P,
                                                        const uint32_t* __restrict__ lbl, int64_t n,
                                                        const F1Image* __restrict__ ip, int nip,
                                                        const uint8_t* __restrict__ ilab, int n_img, int with_pro,
                                                        double* __restrict__ out) {
  // one wave: lane l takes partials l, l + 64, ... in ascending order, then the butterfly. The
  // maximum of a total order does not depend on the order it is searched in.
  F1Best a{-1.0, ~0ull};
  for (int i = threadIdx.x; i < npp; i += 64)
    if (f1_before(pp[i], a)) a = pp[i];
  for (int o = 32; o > 0; o >>= 1) {
    const F1Best other{__shfl_xor(a.f1, o, 64), __shfl_xor(a.pos, o, 64)};
    if (f1_before(other, a)) a = other;
  }
  if (threadIdx.x != 0) return;
  if (!with_pro) out[4] = NAN;
  const uint64_t pos = (uint64_t)P[n - 1] + lbl[n - 1], neg = (uint64_t)n - pos;
  if (pos == 0 || neg == 0 || a.pos >= (uint64_t)n) {  // (block 0 holds position 0, a group start: a.pos is valid)
    out[5] = out[6] = out[7] = out[8] = NAN;
  } else {
    const uint64_t tp = pos - P[a.pos];
    out[5] = a.f1;
    out[6] = (double)ord_value((uint32_t)(keys[a.pos] >> 1));
    out[7] = (double)tp / (double)((uint64_t)n - a.pos);
    out[8] = (double)tp / (double)pos;
  }
  F1Image b = ip[0];
  for (int i = 1; i < nip; ++i)
    if (f1_before(ip[i], b)) b = ip[i];
  uint64_t ipos = 0;
  for (int i = 0; i < n_img; ++i) ipos += ilab[i] != 0;
  if (ipos == 0 || ipos == (uint64_t)n_img) {
    out[9] = out[10] = out[11] = out[12] = 0.0;
  } else {
    out[9] = b.f1;
    out[10] = (double)ord_value(b.key);
    out[11] = (double)b.tp / (double)b.pp;
    out[12] = (double)b.tp / (double)ipos;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Workspace carve-up and the launch sequence, shared by the three entry points: the AUPRO and the
// F1 pieces are appended to the plain layout and to the plain launches, which do not change.
namespace {

struct Layout {  // workspace carve-up (256-B aligned pieces)
  size_t keys_a, keys_b, lbl, gst, P, A, rmin, rmax, fused, norm, ppart, ipart, temp, temp_bytes, total;
  size_t labels, areas, sorted_areas, counts, totals, propart;  // with_pro: the labelling arrays, the sorted areas
  size_t f1part, f1ipart;                                       // with_f1
  int npp, nip;
  int64_t per_block;
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

int plan(int64_t n, int n_img, bool with_pro, bool with_f1, Layout& L) {
  size_t sort_b = 0, scan_b = 0, max_b = 0;
  const hipError_t sq =
      with_pro ? rocprim::radix_sort_pairs((void*)nullptr, sort_b, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                           (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 33)
               : rocprim::radix_sort_keys((void*)nullptr, sort_b, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0,
                                          33);
  if (sq != hipSuccess) return AACLIP_ERR_LAUNCH;
  if (rocprim::exclusive_scan((void*)nullptr, scan_b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n,
                              rocprim::plus<uint32_t>()) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  if (rocprim::inclusive_scan((void*)nullptr, max_b, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n,
                              rocprim::maximum<uint32_t>()) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  L.per_block = 64 * MT;
  L.npp = (int)((n + L.per_block - 1) / L.per_block);
  L.nip = (n_img + MT - 1) / MT;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes);
    return at;
  };
  // keys_a (8 B per pixel) is reused, once sorted into keys_b, for two 4-B arrays
  // (labels, group starts) at 256-B aligned offsets: size it for both aligned halves
  // (8n alone is too small when 4n is not a multiple of 256, e.g. 4 maps of 518^2)
  L.keys_a = take(2 * align_up(4 * (size_t)n));
  L.keys_b = take(8 * (size_t)n);
  L.lbl = L.keys_a;
  L.gst = L.keys_a + align_up(4 * (size_t)n);
  L.P = take(4 * (size_t)n);
  L.A = take(4 * (size_t)n);
  L.rmin = take(4 * (size_t)n_img);
  L.rmax = take(4 * (size_t)n_img);
  L.fused = take(4 * (size_t)n_img);
  L.norm = take(sizeof(Norm));
  L.ppart = take(sizeof(Partial) * (size_t)L.npp);
  L.ipart = take(sizeof(Partial) * (size_t)L.nip);
  if (with_pro) {
    L.labels = L.P;  // component labels are dead once the areas exist, before P is written
    L.areas = take(4 * (size_t)n);
    L.sorted_areas = take(4 * (size_t)n);
    L.counts = take(4 * (size_t)n_img);
    L.totals = take(sizeof(ProTotals));
    L.propart = take(sizeof(double) * (size_t)L.npp);
  }
  if (with_f1) {
    L.f1part = take(sizeof(F1Best) * (size_t)L.npp);
    L.f1ipart = take(sizeof(F1Image) * (size_t)L.nip);
  }
  L.temp_bytes = std::max(sort_b, std::max(scan_b, max_b));
  L.temp = take(L.temp_bytes);
  L.total = o;
  return AACLIP_OK;
}

struct Class {  // one class's operands, checked by the entry point
  const float* pixel_preds;
  const uint8_t* pixel_label;
  const float* image_preds;
  const uint8_t* image_label;
  int n_images;
  int64_t pix_per_image;
  int height, width;  // with_pro only
  int medical;
};

// out[0..3] always; out[4] with_pro (NaN with_f1 alone); out[5..12] with_f1
int launch_metrics(const Class& c, const Layout& L, bool with_pro, double fpr_limit, bool with_f1, void* workspace,
                   double* out, void* stream) {
  const int64_t n = (int64_t)c.n_images * c.pix_per_image;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint64_t* keys_a = (uint64_t*)(ws + L.keys_a);
  uint64_t* keys_b = (uint64_t*)(ws + L.keys_b);
  uint32_t* lbl = (uint32_t*)(ws + L.lbl);
  uint32_t* gst = (uint32_t*)(ws + L.gst);
  uint32_t* P = (uint32_t*)(ws + L.P);
  uint32_t* A = (uint32_t*)(ws + L.A);
  float* rmin = (float*)(ws + L.rmin);
  float* rmax = (float*)(ws + L.rmax);
  float* fused = (float*)(ws + L.fused);
  Norm* nrm = (Norm*)(ws + L.norm);
  Partial* ppart = (Partial*)(ws + L.ppart);
  Partial* ipart = (Partial*)(ws + L.ipart);
  uint32_t* areas = with_pro ? (uint32_t*)(ws + L.areas) : nullptr;
  uint32_t* sorted_areas = with_pro ? (uint32_t*)(ws + L.sorted_areas) : nullptr;
  ProTotals* totals = with_pro ? (ProTotals*)(ws + L.totals) : nullptr;
  void* temp = ws + L.temp;
  size_t tb = L.temp_bytes;

  if (with_pro) {
    uint32_t* counts = (uint32_t*)(ws + L.counts);
    const int rc = aaclip_label_components(c.pixel_label, c.n_images, c.height, c.width, (uint32_t*)(ws + L.labels),
                                           areas, counts, stream);
    if (rc) return rc;
    pro_totals_kernel<<<1, 64, 0, s>>>(counts, c.n_images, totals);
  }
  const int grid = (int)std::min<int64_t>((n + MT - 1) / MT, 4096);
  row_minmax_kernel<<<c.n_images, MT, 0, s>>>(c.pixel_preds, c.pix_per_image, rmin, rmax);
  image_scores_kernel<<<1, MT, 0, s>>>(rmin, rmax, c.image_preds, c.n_images, c.medical, nrm, fused);
  make_keys_kernel<<<grid, MT, 0, s>>>(c.pixel_preds, c.pixel_label, n, nrm, keys_a);
  AACLIP_CHECK_LAUNCH();
  const hipError_t sorted =
      with_pro ? rocprim::radix_sort_pairs(temp, tb, keys_a, keys_b, areas, sorted_areas, (size_t)n, 0, 33, s)
               : rocprim::radix_sort_keys(temp, tb, keys_a, keys_b, (size_t)n, 0, 33, s);
  if (sorted != hipSuccess) return AACLIP_ERR_LAUNCH;
  split_keys_kernel<<<grid, MT, 0, s>>>(keys_b, n, lbl, gst);
  tb = L.temp_bytes;
  if (rocprim::exclusive_scan(temp, tb, lbl, P, 0u, (size_t)n, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  tb = L.temp_bytes;
  if (rocprim::inclusive_scan(temp, tb, gst, A, (size_t)n, rocprim::maximum<uint32_t>(), s) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  pixel_partial_kernel<<<L.npp, MT, 0, s>>>(lbl, P, A, n, L.per_block, ppart);
  image_partial_kernel<<<L.nip, MT, 0, s>>>(fused, c.image_label, c.n_images, ipart);
  finalize_kernel<<<1, 64, 0, s>>>(ppart, L.npp, P, lbl, n, ipart, L.nip, c.image_label, c.n_images, out);
  if (with_pro) {
    double* propart = (double*)(ws + L.propart);
    pro_partial_kernel<<<L.npp, MT, 0, s>>>(lbl, P, A, sorted_areas, n, L.per_block, fpr_limit, propart);
    pro_finalize_kernel<<<1, 64, 0, s>>>(propart, L.npp, P, lbl, n, totals, fpr_limit, out);
  }
  if (with_f1) {  // keys_b is still the sorted keys: nothing above writes it after the sort
    F1Best* f1part = (F1Best*)(ws + L.f1part);
    F1Image* f1ipart = (F1Image*)(ws + L.f1ipart);
    f1_partial_kernel<<<L.npp, MT, 0, s>>>(lbl, P, A, n, L.per_block, f1part);
    f1_image_partial_kernel<<<L.nip, MT, 0, s>>>(fused, c.image_label, c.n_images, f1ipart);
    f1_finalize_kernel<<<1, 64, 0, s>>>(f1part, L.npp, keys_b, P, lbl, n, f1ipart, L.nip, c.image_label, c.n_images,
                                        with_pro ? 1 : 0, out);
  }
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}

int workspace_bytes_for(int64_t n_pixels, int n_images, bool with_pro, bool with_f1, size_t* bytes) {
  AACLIP_REQUIRE(bytes && n_pixels > 0 && n_images > 0 && n_pixels < (1LL << 32) - 1);
  Layout L;
  const int rc = plan(n_pixels, n_images, with_pro, with_f1, L);
  if (rc) return rc;
  *bytes = L.total;
  return AACLIP_OK;
}

}  // namespace

extern "C" int aaclip_metrics_workspace(int64_t n_pixels, int n_images, size_t* bytes) {
  return workspace_bytes_for(n_pixels, n_images, false, false, bytes);
}

extern "C" int aaclip_metrics_eval(const float* pixel_preds, const uint8_t* pixel_label, const float* image_preds,
                                   const uint8_t* image_label, int n_images, int64_t pix_per_image, int medical,
                                   void* workspace, size_t workspace_bytes, double* out, void* stream) {
  AACLIP_REQUIRE(pixel_preds && pixel_label && image_preds && image_label && workspace && out);
  AACLIP_REQUIRE(n_images > 0 && pix_per_image > 0);
  const int64_t n = (int64_t)n_images * pix_per_image;
  AACLIP_REQUIRE(n < (1LL << 32) - 1);
  Layout L;
  const int rc = plan(n, n_images, false, false, L);
  if (rc) return rc;
  AACLIP_REQUIRE(workspace_bytes >= L.total && ((uintptr_t)workspace % 256) == 0);
  const Class c{pixel_preds, pixel_label, image_preds, image_label, n_images, pix_per_image, 0, 0, medical};
  return launch_metrics(c, L, false, 0.0, false, workspace, out, stream);
}

extern "C" int aaclip_metrics_pro_workspace(int64_t n_pixels, int n_images, size_t* bytes) {
  return workspace_bytes_for(n_pixels, n_images, true, false, bytes);
}

extern "C" int aaclip_metrics_eval_pro(const float* pixel_preds, const uint8_t* pixel_label,
                                       const float* image_preds, const uint8_t* image_label, int n_images,
                                       int height, int width, int medical, double fpr_limit, void* workspace,
                                       size_t workspace_bytes, double* out5, void* stream) {
  AACLIP_REQUIRE(pixel_preds && pixel_label && image_preds && image_label && workspace && out5);
  AACLIP_REQUIRE(n_images > 0 && height > 0 && width > 0);
  AACLIP_REQUIRE(fpr_limit > 0.0 && fpr_limit <= 1.0);  // (a NaN fails both)
  const int64_t pix_per_image = (int64_t)height * width;
  AACLIP_REQUIRE(pix_per_image < (1LL << 31));
  const int64_t n = (int64_t)n_images * pix_per_image;
  AACLIP_REQUIRE(n < (1LL << 32) - 1);
  AACLIP_REQUIRE(((uintptr_t)workspace % 256) == 0);
  // keys (8 + 8 B per pixel) and the four 4-B arrays alone: refuse a short workspace before planning
  AACLIP_REQUIRE(workspace_bytes >= 32 * (size_t)n);
  Layout L;
  const int rc = plan(n, n_images, true, false, L);
  if (rc) return rc;
  AACLIP_REQUIRE(workspace_bytes >= L.total);
  const Class c{pixel_preds, pixel_label, image_preds, image_label, n_images, pix_per_image, height, width, medical};
  return launch_metrics(c, L, true, fpr_limit, false, workspace, out5, stream);
}

extern "C" int aaclip_metrics_f1_workspace(int64_t n_pixels, int n_images, int with_pro, size_t* bytes) {
  return workspace_bytes_for(n_pixels, n_images, with_pro != 0, true, bytes);
}

extern "C" int aaclip_metrics_eval_f1(const float* pixel_preds, const uint8_t* pixel_label, const float* image_preds,
                                      const uint8_t* image_label, int n_images, int height, int width, int medical,
                                      int with_pro, double fpr_limit, void* workspace, size_t workspace_bytes,
                                      double* out13, void* stream) {
  AACLIP_REQUIRE(pixel_preds && pixel_label && image_preds && image_label && workspace && out13);
  AACLIP_REQUIRE(n_images > 0 && height > 0 && width > 0);
  AACLIP_REQUIRE(!with_pro || (fpr_limit > 0.0 && fpr_limit <= 1.0));  // (a NaN fails both)
  const int64_t pix_per_image = (int64_t)height * width;
  AACLIP_REQUIRE(pix_per_image < (1LL << 31));
  const int64_t n = (int64_t)n_images * pix_per_image;
  AACLIP_REQUIRE(n < (1LL << 32) - 1);
  AACLIP_REQUIRE(((uintptr_t)workspace % 256) == 0);
  // the keys and the two scans (24 B per pixel), with_pro the areas too (32 B): refuse a short
  // workspace before planning
  AACLIP_REQUIRE(workspace_bytes >= (with_pro ? 32 : 24) * (size_t)n);
  Layout L;
  const int rc = plan(n, n_images, with_pro != 0, true, L);
  if (rc) return rc;
  AACLIP_REQUIRE(workspace_bytes >= L.total);
  const Class c{pixel_preds, pixel_label, image_preds, image_label, n_images, pix_per_image, height, width, medical};
  return launch_metrics(c, L, with_pro != 0, fpr_limit, true, workspace, out13, stream);
}
