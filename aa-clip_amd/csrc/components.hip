// 8-connected component labelling of binary masks on the device (the regions of the
// per-region-overlap metric, aaclip_metrics_eval_pro): label equivalence / union-find in
// global memory, one parent word per pixel, kept in the caller's `labels` array.
//
//   init      one wave per 64-pixel row segment: __ballot of the foreground bit and a bit
//             scan give every pixel the index of its run's first pixel, so the horizontal
//             merges inside a segment cost no memory traffic.
//   merge     the same waves union each run with the segment to its left and with the row
//             above (N, or NW / NE where N is background), once per contact.
//   compress  every pixel finds its root; the root's area word and the image's component
//             count are integer atomicAdds (order-free sums: deterministic), the count
//             gathered per wave over a span of pixels first.
//   publish   labels = 1 + root (the component's smallest linear index: links only ever
//             point from a larger index to a smaller one, so the root is canonical),
//             areas = the root's area.
//
// Unions are lock-free: atomicMin on the larger root's parent word, continued from the
// returned old value until both sides meet. Parents only decrease, so every loop ends on
// its own; no wave ever waits for another. Parent reads are relaxed agent-scope atomic
// loads (the per-CU L1 is not refreshed by other CUs' atomics); a stale parent would only
// cost an extra round, because atomicMin returns the true word. Every loop that follows
// memory other waves write also carries a hard cap of H*W trips; hitting it sets bit 31 of
// the image's count (a count is < 2^31), published as 0xFFFFFFFF: a bug ends in a wrong
// number, never in a hang.
#include "common.h"
#include "rowseg.h"

namespace {

constexpr uint32_t BG = 0xFFFFFFFFu;
constexpr uint32_t CAP_HIT = 0x80000000u;

__device__ __forceinline__ uint32_t parent_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Follows parents down to a root. Only ever steps to a smaller index, so it stays inside
// the image whatever it reads; `cap` bounds the walk.
__device__ __forceinline__ uint32_t find_root(const uint32_t* par, uint32_t x, uint32_t cap, bool& capped) {
  for (uint32_t it = 0; it < cap; ++it) {
    const uint32_t p = parent_load(par + x);
    if (p >= x) return x;
    x = p;
  }
  capped = true;
  return x;
}

__device__ __forceinline__ void unite(uint32_t* par, uint32_t a, uint32_t b, uint32_t cap, bool& capped) {
  for (uint32_t it = 0; it < cap; ++it) {
    a = find_root(par, a, cap, capped);
    b = find_root(par, b, cap, capped);
    if (a == b || capped) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(par + a, b);  // link the larger root under the smaller
    if (old == a) return;                        // a was still a root: linked
    a = old;                                     // a had a parent already (old < a): go on from it
  }
  capped = true;
}

__global__ __launch_bounds__(CT) void cc_init_kernel(const uint8_t* __restrict__ mask, int n, int H, int W,
                                                     uint32_t* __restrict__ par, uint32_t* __restrict__ areas,
                                                     uint32_t* __restrict__ counts) {
  const Segment s = my_segment(n, H, W);
  if (!s.valid) return;  // whole wave
  const int x = s.x0 + s.lane;
  const bool in = x < W;
  const size_t at = s.base + (size_t)s.y * W + (in ? x : 0);
  const bool fg = in && mask[at] != 0;
  const uint64_t row = __ballot(fg);
  if (in) {
    uint32_t p = BG;
    if (fg) p = (uint32_t)(s.y * W + s.x0 + run_start(row, s.lane));  // first pixel of this lane's run
    par[at] = p;
    areas[at] = 0u;
  }
  if (s.y == 0 && s.x0 == 0 && s.lane == 0) counts[s.img] = 0u;
}

__global__ __launch_bounds__(CT) void cc_merge_kernel(const uint8_t* __restrict__ mask, int n, int H, int W,
                                                      uint32_t* __restrict__ parents, uint32_t* __restrict__ counts) {
  const Segment s = my_segment(n, H, W);
  if (!s.valid) return;  // whole wave
  const uint8_t* m = mask + s.base;
  uint32_t* par = parents + s.base;
  const int x = s.x0 + s.lane, y = s.y;
  const bool in = x < W;
  const size_t rowat = (size_t)y * W, upat = rowat - (y > 0 ? W : 0);
  const bool fg = in && m[rowat + x] != 0;
  const bool up = y > 0 && in && m[upat + x] != 0;
  const uint64_t row = __ballot(fg), above = __ballot(up);
  if (!row) return;
  // the three pixels just outside the segment that its end lanes touch (never across the
  // image's left / right border: x0 - 1 and x0 + 64 are columns of the same row)
  const bool left = s.x0 > 0 && m[rowat + s.x0 - 1] != 0;
  const bool up_left = y > 0 && s.x0 > 0 && m[upat + s.x0 - 1] != 0;
  const bool up_right = y > 0 && s.x0 + 64 < W && m[upat + s.x0 + 64] != 0;
  if (!fg) return;
  const int l = s.lane;
  const bool prev = l ? (row >> (l - 1)) & 1 : left;
  const bool next = l < 63 ? (row >> (l + 1)) & 1 : false;
  const bool nn = (above >> l) & 1;
  const bool nw = l ? (above >> (l - 1)) & 1 : up_left;
  const bool ne = l < 63 ? (above >> (l + 1)) & 1 : up_right;
  const uint32_t p = (uint32_t)(rowat + x), cap = (uint32_t)(H * W);
  bool capped = false;
  if (l == 0 && left) unite(par, p, p - 1, cap, capped);
  if (nn) {
    // the first pixel of a contact joins the two runs; the previous pixel did it otherwise
    if (!(prev && nw)) unite(par, p, p - (uint32_t)W, cap, capped);
  } else {
    if (nw) unite(par, p, p - (uint32_t)W - 1, cap, capped);
    if (ne && !next) unite(par, p, p - (uint32_t)W + 1, cap, capped);  // (with next set, it has N = this NE)
  }
  if (capped) atomicOr(counts + s.img, CAP_HIT);
}

// Every wave walks a contiguous span of the class's pixels, 64 at a time (`span` is a multiple of
// 64). Parents become roots; each wave adds its pixels to their roots' area words, one atomicAdd per
// distinct root in the 64 pixels. The roots it meets are counted in a register and added to the
// image's count when the span leaves the image or ends: a few adds per wave, where one add per
// root put every component of an image in line on one address (thousands, when a threshold leaves
// a noisy map in specks).
__global__ __launch_bounds__(CT) void cc_compress_kernel(int64_t total, uint32_t hw, int64_t span,
                                                         uint32_t* __restrict__ parents,
                                                         uint32_t* __restrict__ areas,
                                                         uint32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t begin = ((int64_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6)) * span;
  const int64_t end = begin + span < total ? begin + span : total;
  uint32_t held_img = 0u, held = 0u;  // wave-uniform: roots seen in held_img and not yet added
  for (int64_t at = begin; at < end; at += 64) {  // wave-uniform
    const int64_t i = at + lane;
    const bool in = i < end;
    const uint32_t img = in ? (uint32_t)(i / hw) : 0u;
    const uint32_t p = in ? (uint32_t)(i - (int64_t)img * hw) : 0u;
    const size_t base = (size_t)img * hw;
    const bool fg = in && parent_load(parents + base + p) != BG;
    uint32_t groot = BG;  // root as an index into the whole class (n * H * W < 2^32 - 1)
    bool is_root = false;
    if (fg) {
      bool capped = false;
      const uint32_t r = find_root(parents + base, p, hw, capped);
      __hip_atomic_store(parents + base + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      groot = (uint32_t)(base + r);
      is_root = r == p;
      if (capped) atomicOr(counts + img, CAP_HIT);
    }
    uint64_t todo = __ballot(fg);
    while (todo) {  // wave-uniform; every trip retires at least the leader
      const int lead = __ffsll((unsigned long long)todo) - 1;
      const uint32_t r0 = __shfl(groot, lead, 64);
      const uint64_t same = __ballot(fg && groot == r0);
      if (lane == lead) atomicAdd(areas + r0, (uint32_t)__popcll(same));
      todo &= ~same;
    }
    uint64_t roots = __ballot(is_root);
    while (roots) {  // wave-uniform; one trip per image among the 64 pixels' roots
      const int lead = __ffsll((unsigned long long)roots) - 1;
      const uint32_t im = __shfl(img, lead, 64);
      const uint64_t same = __ballot(is_root && img == im);
      if (im != held_img) {
        if (held && lane == 0) atomicAdd(counts + held_img, held);
        held_img = im;
        held = 0u;
      }
      held += (uint32_t)__popcll(same);
      roots &= ~same;
    }
  }
  if (held && lane == 0) atomicAdd(counts + held_img, held);
}

__global__ __launch_bounds__(CT) void cc_publish_kernel(int64_t total, uint32_t hw, uint32_t* __restrict__ labels,
                                                        uint32_t* __restrict__ areas,
                                                        uint32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (i >= total) return;
  const uint32_t img = (uint32_t)(i / hw);
  const uint32_t p = (uint32_t)(i - (int64_t)img * hw);
  const uint32_t r = labels[i];
  if (r == BG) {
    labels[i] = 0u;
  } else {
    if (r != p) areas[i] = areas[(size_t)img * hw + r];  // only root words hold a sum; nobody reads the others
    labels[i] = r + 1u;
  }
  if (p == 0 && (counts[img] & CAP_HIT)) counts[img] = 0xFFFFFFFFu;
}

}  // namespace

extern "C" int aaclip_label_components(const uint8_t* mask, int n_images, int height, int width, uint32_t* labels,
                                       uint32_t* areas, uint32_t* n_components, void* stream) {
  AACLIP_REQUIRE(mask && labels && areas && n_components);
  AACLIP_REQUIRE(n_images > 0 && height > 0 && width > 0);
  const int64_t hw = (int64_t)height * width;
  AACLIP_REQUIRE(hw < (1LL << 31));
  const int64_t total = (int64_t)n_images * hw;
  AACLIP_REQUIRE(total < (1LL << 32) - 1);
  hipStream_t s = (hipStream_t)stream;
  const int64_t waves = (int64_t)n_images * height * ((width + 63) / 64);
  const unsigned seg_grid = (unsigned)((waves + CT / 64 - 1) / (CT / 64));
  const unsigned pix_grid = (unsigned)((total + CT - 1) / CT);
  cc_init_kernel<<<seg_grid, CT, 0, s>>>(mask, n_images, height, width, labels, areas, n_components);
  cc_merge_kernel<<<seg_grid, CT, 0, s>>>(mask, n_images, height, width, labels, n_components);
  // 8192 waves at most, each over a 64-aligned span: a count takes a few adds per wave
  const int64_t span = ((total + 8192 * 64 - 1) / (8192 * 64)) * 64;
  const unsigned span_grid = (unsigned)(((total + span - 1) / span + CT / 64 - 1) / (CT / 64));
  cc_compress_kernel<<<span_grid, CT, 0, s>>>(total, (uint32_t)hw, span, labels, areas, n_components);
  cc_publish_kernel<<<pix_grid, CT, 0, s>>>(total, (uint32_t)hw, labels, areas, n_components);
  AACLIP_CHECK_LAUNCH();
  return AACLIP_OK;
}
