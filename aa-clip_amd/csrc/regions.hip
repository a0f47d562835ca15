// Defect regions of the anomaly maps on the device (aaclip_extract_regions): apply a threshold to
// the class-normalised score, label the 8-connected components of what is left
// (aaclip_label_components), and give every component its area, bounding box, centroid, peak and
// overlap with the ground truth, the largest first.
//
//   foreground  v >= threshold, v the score of scorenorm.h (the metrics' normalisation, or the
//               raw value); a NaN compares false and is background.
//   label       components.hip; labels = 1 + root, areas = the root's area, per pixel.
//   compact     the roots that pass min_area are flagged and scanned (rocPRIM): a root's rank in
//               the scan is its slot in the per-region arrays, and the scan value at an image's
//               first pixel is the image's first slot. At most ceil(H/2) ceil(W/2) components fit
//               an image, so the slot arrays are a quarter of the pixel arrays.
//   accumulate  one wave per 64-pixel row segment, as the labelling: a run of adjacent foreground
//               pixels belongs to one region, its first lane gets the run's peak by a segmented
//               shuffle scan and everything else (x range, sum of x, length, ground-truth count)
//               from the ballot words in closed form, and updates the slot: min / max / add on
//               32- and 64-bit integers, one set per run. The peak and its first index are one
//               64-bit max on (ord_bits(v) << 32) | ~index. Integer atomics commute: the same
//               bits whatever the order.
//   sort        one radix sort of all slots by (image, area descending, label ascending) packed
//               as ((image hw + hw - area) hw + label - 1) < n hw^2 < 2^63; unused slots hold
//               n hw^2 and sort last. Its size is the slot capacity, known on the host: no count
//               is read back and nothing syncs.
//   emit        one thread per output slot decodes label and area from the sorted key, divides
//               the sums (one fp64 division each) and zero-fills past the count.
//
// Every index that comes from data (labels, ranks, sorted values) is compared with its array's
// size before use; no loop here depends on data.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "rowseg.h"
#include "scorenorm.h"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
typedef unsigned long long u64;

// the class's Norm from the per-image extremes (normalise == 0: the identity)
__global__ __launch_bounds__(MT) void class_norm_kernel(const float* __restrict__ rmin,
                                                        const float* __restrict__ rmax, int n_img, int normalise,
                                                        Norm* __restrict__ nrm) {
  __shared__ float sh[MT / 64];
  if (!normalise) {  // whole block
    if (threadIdx.x == 0) *nrm = Norm{0.f, 0.f, 0.f, 0.f, 0, 0};
    return;
  }
  float lo, hi;
  class_minmax(rmin, rmax, n_img, sh, lo, hi);
  if (threadIdx.x == 0) *nrm = Norm{lo, hi, 0.f, 0.f, norm_wanted(hi), 0};
}

__global__ __launch_bounds__(MT) void foreground_kernel(const float* __restrict__ p, int64_t total,
                                                        const Norm* __restrict__ nrm, float threshold,
                                                        uint8_t* __restrict__ mask) {
  const Norm z = *nrm;
  for (int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x; i < total; i += (int64_t)gridDim.x * MT)
    mask[i] = pixel_score(p[i], z) >= threshold ? 1 : 0;  // (false for a NaN)
}

// flag = 1 at the root pixel of every component that passes min_area
__global__ __launch_bounds__(MT) void root_flags_kernel(const uint32_t* __restrict__ labels,
                                                        const uint32_t* __restrict__ areas, int64_t total,
                                                        uint32_t hw, uint32_t min_area,
                                                        uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (i >= total) return;
  const uint32_t p = (uint32_t)(i % hw);
  flag[i] = labels[i] == p + 1u && areas[i] >= min_area ? 1u : 0u;
}

struct Slots {  // per-region arrays, `cap` entries each
  uint32_t cap;
  u64* keys;  // sort key
  uint32_t* vals;  // the slot's own index, carried through the sort
  uint32_t *x0, *x1, *y1, *gt;
  u64 *sumx, *sumy, *peak;
};

// One thread per pixel: kept roots open their slot, unused slots get the padding key, and the
// image's first slot is noted (first[n_img] = the number of slots in use).
__global__ __launch_bounds__(MT) void open_slots_kernel(const uint32_t* __restrict__ areas,
                                                        const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ rank, int64_t total,
                                                        uint32_t hw, int n_img, Slots S,
                                                        uint32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (i >= total) return;
  const uint32_t used = rank[total - 1] + flag[total - 1];
  const uint32_t img = (uint32_t)(i / hw), p = (uint32_t)(i % hw);
  if (p == 0) first[img] = rank[i];
  if (i == total - 1) first[n_img] = used;
  if (i < (int64_t)S.cap && i >= (int64_t)used) {
    S.keys[i] = (u64)total * hw;
    S.vals[i] = (uint32_t)i;
  }
  if (!flag[i]) return;
  const uint32_t j = rank[i];
  if (j >= S.cap) return;  // (more roots than an image can hold: never, unless there is a bug)
  S.keys[j] = ((u64)img * hw + (hw - areas[i])) * hw + p;
  S.vals[j] = j;
  S.x0[j] = NONE;
  S.x1[j] = S.y1[j] = S.gt[j] = 0u;
  S.sumx[j] = S.sumy[j] = S.peak[j] = 0ull;
}

__global__ __launch_bounds__(CT) void accumulate_kernel(const float* __restrict__ preds,
                                                        const uint8_t* __restrict__ gt_label,
                                                        const uint32_t* __restrict__ labels,
                                                        const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ rank,
                                                        const Norm* __restrict__ nrm, int n, int H, int W, Slots S) {
  const Segment s = my_segment(n, H, W);
  if (!s.valid) return;  // whole wave
  const int x = s.x0 + s.lane, l = s.lane;
  const bool in = x < W;
  const uint32_t p = (uint32_t)(s.y * W + (in ? x : 0));
  const size_t at = s.base + p;
  const uint32_t lab = in ? labels[at] : 0u;
  uint32_t slot = NONE;
  if (lab != 0u && lab <= (uint32_t)(H * W)) {
    const size_t r = s.base + (lab - 1u);
    if (flag[r]) slot = rank[r];
    if (slot >= S.cap) slot = NONE;
  }
  const bool keep = slot != NONE;
  const uint64_t row = __ballot(keep);
  if (!row) return;
  const uint64_t truth = __ballot(keep && gt_label != nullptr && gt_label[at] != 0);
  // adjacent foreground pixels are one component: the run [start, end] of this lane shares its slot
  const int start = run_start(row, l);
  const uint64_t above = ~row & ~((2ull << l) - 1ull);  // (lane 63: 2 << 63 wraps to 0, no bit is above)
  const int end = above ? __ffsll((unsigned long long)above) - 2 : 63;
  u64 best = 0ull;
  if (keep) best = ((u64)ord_bits(pixel_score(preds[at], *nrm)) << 32) | (u64)(~p);
  for (int o = 1; o < 64; o <<= 1) {  // suffix maximum within the run: lane `start` ends with the run's
    const u64 other = __shfl_down(best, o, 64);
    if (keep && l + o <= end && other > best) best = other;
  }
  if (!keep || l != start) return;
  const uint32_t xs = (uint32_t)(s.x0 + start), xe = (uint32_t)(s.x0 + end), len = xe - xs + 1u;
  const uint64_t run = (end == 63 ? ~0ull : (2ull << end) - 1ull) & ~((1ull << start) - 1ull);
  const uint32_t hits = (uint32_t)__popcll(truth & run);
  atomicMin(S.x0 + slot, xs);
  atomicMax(S.x1 + slot, xe);
  atomicMax(S.y1 + slot, (uint32_t)s.y);
  atomicAdd(S.sumx + slot, (u64)(xs + xe) * len / 2ull);
  atomicAdd(S.sumy + slot, (u64)s.y * len);
  atomicMax(S.peak + slot, best);
  if (hits) atomicAdd(S.gt + slot, hits);
}

struct Outputs {
  uint32_t *n_regions, *label, *area, *bbox;
  double* centroid;
  float* peak;
  uint32_t *peak_index, *gt_area;
};

// One thread per output slot [image, j].
__global__ __launch_bounds__(MT) void emit_kernel(int n_img, int max_regions, uint32_t hw, uint32_t W,
                                                  const uint32_t* __restrict__ counts,
                                                  const uint32_t* __restrict__ first,
                                                  const u64* __restrict__ sorted_keys,
                                                  const uint32_t* __restrict__ sorted_vals, Slots S, Outputs O) {
  const int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (t >= (int64_t)n_img * max_regions) return;
  const int img = (int)(t / max_regions), j = (int)(t % max_regions);
  const bool failed = counts[img] == 0xFFFFFFFFu;  // a labelling cap was hit: passed through
  const uint32_t begin = first[img], count = first[img + 1] - begin;
  if (j == 0) O.n_regions[img] = failed ? 0xFFFFFFFFu : count;
  const uint32_t pos = begin + (uint32_t)j;
  bool have = !failed && (uint32_t)j < count && pos < S.cap;
  uint32_t slot = have ? sorted_vals[pos] : NONE;
  have = have && slot < S.cap;
  uint32_t label = 0, area = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0, peak_index = 0, gt = 0;
  double cx = 0.0, cy = 0.0;
  float peak = 0.f;
  if (have) {
    const u64 key = sorted_keys[pos];
    label = (uint32_t)(key % hw) + 1u;
    area = hw - (uint32_t)((key / hw) % hw);
    x0 = S.x0[slot];
    y0 = (label - 1u) / W;  // the root is the region's smallest linear index: its row is the top row
    x1 = S.x1[slot];
    y1 = S.y1[slot];
    cx = (double)S.sumx[slot] / (double)area;
    cy = (double)S.sumy[slot] / (double)area;
    const u64 best = S.peak[slot];
    peak = ord_value((uint32_t)(best >> 32));
    peak_index = ~(uint32_t)best;
    gt = S.gt[slot];
  }
  O.label[t] = label;
  O.area[t] = area;
  O.bbox[4 * t + 0] = x0;
  O.bbox[4 * t + 1] = y0;
  O.bbox[4 * t + 2] = x1;
  O.bbox[4 * t + 3] = y1;
  O.centroid[2 * t + 0] = cx;
  O.centroid[2 * t + 1] = cy;
  O.peak[t] = peak;
  O.peak_index[t] = peak_index;
  O.gt_area[t] = gt;
}

struct Layout {  // workspace carve-up (256-B aligned pieces)
  size_t rmin, rmax, norm, mask, labels, areas, flag, rank, counts, first;
  size_t keys_a, keys_b, vals_a, vals_b, x0, x1, y1, gt, sumx, sumy, peak;
  size_t temp, temp_bytes, total;
  uint32_t cap;  // slots the arrays hold: what any [height, width] of this pixel count can need
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

int sort_temp_bytes(size_t count, unsigned bits, size_t& bytes) {
  bytes = 0;
  return rocprim::radix_sort_pairs((void*)nullptr, bytes, (u64*)nullptr, (u64*)nullptr, (uint32_t*)nullptr,
                                   (uint32_t*)nullptr, count, 0, bits) == hipSuccess
             ? AACLIP_OK
             : AACLIP_ERR_LAUNCH;
}

int plan(int64_t n, int n_img, Layout& L) {
  const int64_t hw = n / n_img;
  // an image of hw pixels holds at most (hw + 1) / 2 components (a single row, every other pixel)
  L.cap = (uint32_t)((int64_t)n_img * ((hw + 1) / 2));
  size_t sort_b = 0, scan_b = 0;
  if (sort_temp_bytes(L.cap, 64, sort_b)) return AACLIP_ERR_LAUNCH;
  if (rocprim::exclusive_scan((void*)nullptr, scan_b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n,
                              rocprim::plus<uint32_t>()) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes);
    return at;
  };
  L.rmin = take(4 * (size_t)n_img);
  L.rmax = take(4 * (size_t)n_img);
  L.norm = take(sizeof(Norm));
  L.mask = take((size_t)n);
  L.labels = take(4 * (size_t)n);
  L.areas = take(4 * (size_t)n);
  L.flag = take(4 * (size_t)n);
  L.rank = take(4 * (size_t)n);
  L.counts = take(4 * (size_t)n_img);
  L.first = take(4 * ((size_t)n_img + 1));
  const size_t c = L.cap;
  L.keys_a = take(8 * c);
  L.keys_b = take(8 * c);
  L.vals_a = take(4 * c);
  L.vals_b = take(4 * c);
  L.x0 = take(4 * c);
  L.x1 = take(4 * c);
  L.y1 = take(4 * c);
  L.gt = take(4 * c);
  L.sumx = take(8 * c);
  L.sumy = take(8 * c);
  L.peak = take(8 * c);
  L.temp_bytes = std::max(sort_b, scan_b);
  L.temp = take(L.temp_bytes);
  L.total = o;
  return AACLIP_OK;
}

}  // namespace

extern "C" int aaclip_regions_workspace(int64_t n_pixels, int n_images, size_t* bytes) {
  AACLIP_REQUIRE(bytes && n_pixels > 0 && n_images > 0 && n_pixels < (1LL << 32) - 1);
  AACLIP_REQUIRE(n_pixels % n_images == 0 && n_pixels / n_images < (1LL << 31));
  Layout L;
  const int rc = plan(n_pixels, n_images, L);
  if (rc) return rc;
  *bytes = L.total;
  return AACLIP_OK;
}

extern "C" int aaclip_extract_regions(const float* pixel_preds, const uint8_t* pixel_label, int n_images, int height,
                                      int width, float threshold, int normalise, int min_area, int max_regions,
                                      void* workspace, size_t workspace_bytes, uint32_t* n_regions,
                                      uint32_t* labels, uint32_t* areas, uint32_t* bboxes, double* centroids,
                                      float* peaks, uint32_t* peak_indices, uint32_t* gt_areas, void* stream) {
  AACLIP_REQUIRE(pixel_preds && workspace && n_regions && labels && areas && bboxes && centroids && peaks &&
                 peak_indices && gt_areas);
  AACLIP_REQUIRE(n_images > 0 && height > 0 && width > 0 && min_area >= 1 && max_regions >= 1);
  const int64_t hw = (int64_t)height * width;
  AACLIP_REQUIRE(hw < (1LL << 31));
  const int64_t total = (int64_t)n_images * hw;
  AACLIP_REQUIRE(total < (1LL << 32) - 1);
  AACLIP_REQUIRE((int64_t)n_images * max_regions < (1LL << 31));
  AACLIP_REQUIRE(((uintptr_t)workspace % 256) == 0);
  AACLIP_REQUIRE(workspace_bytes >= 17 * (size_t)total);  // the pixel arrays alone: refuse before planning
  Layout L;
  int rc = plan(total, n_images, L);
  if (rc) return rc;
  AACLIP_REQUIRE(workspace_bytes >= L.total);
  // the slots this shape can need, and the bits of the padding key n hw^2, the largest one
  const uint32_t cap = (uint32_t)((int64_t)n_images * ((height + 1) / 2) * ((width + 1) / 2));
  AACLIP_REQUIRE(cap <= L.cap);
  const unsigned bits = 64u - (unsigned)__builtin_clzll((unsigned long long)total * (unsigned long long)hw);
  size_t sort_b = 0;
  if (sort_temp_bytes(cap, bits, sort_b)) return AACLIP_ERR_LAUNCH;
  AACLIP_REQUIRE(sort_b <= L.temp_bytes);

  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* rmin = (float*)(ws + L.rmin);
  float* rmax = (float*)(ws + L.rmax);
  Norm* nrm = (Norm*)(ws + L.norm);
  uint8_t* mask = (uint8_t*)(ws + L.mask);
  uint32_t* comp = (uint32_t*)(ws + L.labels);
  uint32_t* comp_area = (uint32_t*)(ws + L.areas);
  uint32_t* flag = (uint32_t*)(ws + L.flag);
  uint32_t* rank = (uint32_t*)(ws + L.rank);
  uint32_t* counts = (uint32_t*)(ws + L.counts);
  uint32_t* first = (uint32_t*)(ws + L.first);
  u64* keys_b = (u64*)(ws + L.keys_b);
  uint32_t* vals_b = (uint32_t*)(ws + L.vals_b);
  const Slots S{cap,
                (u64*)(ws + L.keys_a),
                (uint32_t*)(ws + L.vals_a),
                (uint32_t*)(ws + L.x0),
                (uint32_t*)(ws + L.x1),
                (uint32_t*)(ws + L.y1),
                (uint32_t*)(ws + L.gt),
                (u64*)(ws + L.sumx),
                (u64*)(ws + L.sumy),
                (u64*)(ws + L.peak)};
  const Outputs O{n_regions, labels, areas, bboxes, centroids, peaks, peak_indices, gt_areas};
  void* temp = ws + L.temp;

  const int grid = (int)std::min<int64_t>((total + MT - 1) / MT, 4096);
  const unsigned pix_grid = (unsigned)((total + MT - 1) / MT);
  const int64_t waves = (int64_t)n_images * height * ((width + 63) / 64);
  const unsigned seg_grid = (unsigned)((waves + CT / 64 - 1) / (CT / 64));
  if (normalise) row_minmax_kernel<<<n_images, MT, 0, s>>>(pixel_preds, hw, rmin, rmax);
  class_norm_kernel<<<1, MT, 0, s>>>(rmin, rmax, n_images, normalise, nrm);
  foreground_kernel<<<grid, MT, 0, s>>>(pixel_preds, total, nrm, threshold, mask);
  AACLIP_CHECK_LAUNCH();
  rc = aaclip_label_components(mask, n_images, height, width, comp, comp_area, counts, stream);
  if (rc) return rc;
  root_flags_kernel<<<pix_grid, MT, 0, s>>>(comp, comp_area, total, (uint32_t)hw, (uint32_t)min_area, flag);
  size_t tb = L.temp_bytes;
  if (rocprim::exclusive_scan(temp, tb, flag, rank, 0u, (size_t)total, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  open_slots_kernel<<<pix_grid, MT, 0, s>>>(comp_area, flag, rank, total, (uint32_t)hw, n_images, S, first);
  accumulate_kernel<<<seg_grid, CT, 0, s>>>(pixel_preds, pixel_label, comp, flag, rank, nrm, n_images, height, width,
                                            S);
  AACLIP_CHECK_LAUNCH();
  tb = L.temp_bytes;
  if (rocprim::radix_sort_pairs(temp, tb, S.keys, keys_b, S.vals, vals_b, (size_t)cap, 0, bits, s) != hipSuccess)
    return AACLIP_ERR_LAUNCH;
  const unsigned out_grid = (unsigned)(((int64_t)n_images * max_regions + MT - 1) / MT);
  emit_kernel<<<out_grid, MT, 0, s>>>(n_images, max_regions, (uint32_t)hw, (uint32_t)width, counts, first, keys_b,
                                      vals_b, S, O);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
