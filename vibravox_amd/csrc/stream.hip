// Streaming inference: a layer's input for this push, assembled from the previous push's buffer and the producer's fresh output.
//
//   dst[rc, j]           = prev[rc, prev_off + j]                         j < n_carry
//   dst[rc, n_carry + j] = src[rc, src_off + j] (+ add[rc, add_off + j])  j < n_new
//
// rc runs over rows x channels of fp32 [row][C][L] tensors, each with its own row pitch; offsets and counts are arbitrary (scalar
// loads and stores: nothing assumes a 16-byte grid).  dst never aliases a source -- the carry is usually longer than the new part,
// so a shift in place would race; the caller ping-pongs two buffers.  The entry checks every range against its pitch and the four
// extents against each other before it launches: a bad call fails on the host and writes nothing.
//
// Independent sessions (streaming.StreamPool) share one state of `slots` rows, and only some of them push in a tick:
// eben_stream_splice_rows is the splice with a slot dimension and a mask of the slots that advance, handed over by value (no device
// mask buffer).  With a = the number of active slots below r, an active slot r does what the plain splice does for its row, reading
// src / add at row a when they are compact (one row per ACTIVE slot) and writing dst at row a when it is; an inactive slot copies
// idle[r] to dst[r] when idle is given (its state moves to the twin buffer unchanged: the ping-pong parity stays global) and writes
// nothing otherwise.  eben_copy_segments moves a session between its private state and a slot: up to 64 contiguous (dst, src, floats)
// segments, the table by value, one launch.
#include "common.h"

namespace eben {
namespace {

// thread = one element of dst, consecutive threads consecutive positions of one (row, channel)
__global__ __launch_bounds__(256) void stream_splice_kernel(float* __restrict__ dst, int dst_pitch, const float* __restrict__ prev, int prev_pitch,
                                                            int prev_off, int n_carry, const float* __restrict__ src, int src_pitch, int src_off,
                                                            int n_new, const float* __restrict__ add, int add_pitch, int add_off, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int len = n_carry + n_new;
  const long long rc = idx / len;
  const int j = (int)(idx - rc * len);
  float v;
  if (j < n_carry) {
    v = prev[rc * prev_pitch + prev_off + j];
  } else {
    const int k = j - n_carry;
    v = src[rc * src_pitch + src_off + k];
    if (add) v += add[rc * add_pitch + add_off + k];
  }
  dst[rc * dst_pitch + j] = v;
}

struct SlotMask { unsigned long long w[4]; };   // EBEN_STREAM_MAX_SLOTS bits

// thread = one element of [carry | new] of one (slot, channel); the per-slot decision is uniform over a row, so nearly over a wave
__global__ __launch_bounds__(256) void stream_splice_rows_kernel(float* __restrict__ dst, int dst_pitch, const float* __restrict__ prev, int prev_pitch,
                                                                 int prev_off, int n_carry, const float* __restrict__ src, int src_pitch, int src_off,
                                                                 int n_new, const float* __restrict__ add, int add_pitch, int add_off,
                                                                 const float* __restrict__ idle, int idle_pitch, int channels, SlotMask mask,
                                                                 int src_compact, int dst_compact, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int len = n_carry + n_new;
  const long long rc = idx / len;
  const int j = (int)(idx - rc * len);
  const int r = (int)(rc / channels), c = (int)(rc - (long long)r * channels);
  const int word = r >> 6, bit = r & 63;
  const unsigned long long mw = mask.w[word];
  if (!((mw >> bit) & 1ull)) {
    if (idle && !dst_compact) dst[rc * dst_pitch + j] = idle[rc * idle_pitch + j];
    return;
  }
  int a = __popcll(mw & ((1ull << bit) - 1ull));
  for (int q = 0; q < word; ++q) a += __popcll(mask.w[q]);
  const long long in_rc = src_compact ? (long long)a * channels + c : rc;
  const long long out_rc = dst_compact ? (long long)a * channels + c : rc;
  float v;
  if (j < n_carry) {
    v = prev[rc * prev_pitch + prev_off + j];
  } else {
    const int k = j - n_carry;
    v = src[in_rc * src_pitch + src_off + k];
    if (add) v += add[in_rc * add_pitch + add_off + k];
  }
  dst[out_rc * dst_pitch + j] = v;
}

struct SegmentTable { EbenCopySegment s[EBEN_COPY_MAX_SEGMENTS]; };

// blockIdx.y = segment, the blocks of a row stride over its floats
__global__ __launch_bounds__(256) void copy_segments_kernel(SegmentTable t) {
  const EbenCopySegment seg = t.s[blockIdx.y];
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < seg.floats; i += step) seg.dst[i] = seg.src[i];
}

inline bool overlaps(const float* a, long long na, const float* b, long long nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + 4ull * (unsigned long long)nb && b0 < a0 + 4ull * (unsigned long long)na;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_stream_splice(float* dst, int dst_pitch, const float* prev, int prev_pitch, int prev_off, int n_carry, const float* src,
                                  int src_pitch, int src_off, int n_new, const float* add, int add_pitch, int add_off, int rows_channels,
                                  void* stream) {
  EBEN_REQUIRE(dst, "stream_splice: null dst");
  EBEN_REQUIRE(rows_channels > 0 && n_carry >= 0 && n_new >= 0 && (long long)n_carry + n_new > 0, "stream_splice: %d rows x channels, carry %d, new %d",
               rows_channels, n_carry, n_new);
  EBEN_REQUIRE(dst_pitch > 0 && (long long)n_carry + n_new <= dst_pitch, "stream_splice: carry %d + new %d past dst's pitch %d", n_carry, n_new, dst_pitch);
  EBEN_REQUIRE(n_carry == 0 || prev, "stream_splice: null prev with a carry of %d", n_carry);
  EBEN_REQUIRE(n_new == 0 || src, "stream_splice: null src with %d new samples", n_new);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(add);
  EBEN_REQUIRE((bits & 3) == 0, "stream_splice: misaligned pointer");
  if (n_carry > 0)
    EBEN_REQUIRE(prev_pitch > 0 && prev_off >= 0 && (long long)prev_off + n_carry <= prev_pitch, "stream_splice: prev offset %d + carry %d past its pitch %d",
                 prev_off, n_carry, prev_pitch);
  if (n_new > 0) {
    EBEN_REQUIRE(src_pitch > 0 && src_off >= 0 && (long long)src_off + n_new <= src_pitch, "stream_splice: src offset %d + new %d past its pitch %d", src_off,
                 n_new, src_pitch);
    if (add)
      EBEN_REQUIRE(add_pitch > 0 && add_off >= 0 && (long long)add_off + n_new <= add_pitch, "stream_splice: add offset %d + new %d past its pitch %d", add_off,
                   n_new, add_pitch);
  }
  const long long rc = rows_channels;
  if (n_carry > 0) EBEN_REQUIRE(!overlaps(dst, rc * dst_pitch, prev, rc * prev_pitch), "stream_splice: dst overlaps prev");
  if (n_new > 0) {
    EBEN_REQUIRE(!overlaps(dst, rc * dst_pitch, src, rc * src_pitch), "stream_splice: dst overlaps src");
    if (add) EBEN_REQUIRE(!overlaps(dst, rc * dst_pitch, add, rc * add_pitch), "stream_splice: dst overlaps add");
  }
  const long long total = rc * ((long long)n_carry + n_new);
  const long long blocks = (total + 255) / 256;
  EBEN_REQUIRE(blocks <= 0x7fffffffLL, "stream_splice: grid of %lld blocks", blocks);
  hipLaunchKernelGGL(stream_splice_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dst, dst_pitch, prev, prev_pitch, prev_off, n_carry,
                     src, src_pitch, src_off, n_new, add, add_pitch, add_off, total);
  EBEN_CHECK_LAUNCH("stream_splice_kernel");
  return EBEN_OK;
}

extern "C" int eben_stream_splice_rows(float* dst, int dst_pitch, const float* prev, int prev_pitch, int prev_off, int n_carry, const float* src,
                                       int src_pitch, int src_off, int n_new, const float* add, int add_pitch, int add_off, const float* idle,
                                       int idle_pitch, int rows_channels, int channels, const unsigned long long* active, int src_compact,
                                       int dst_compact, void* stream) {
  EBEN_REQUIRE(dst, "stream_splice_rows: null dst");
  EBEN_REQUIRE(active, "stream_splice_rows: null active mask");
  EBEN_REQUIRE(rows_channels > 0 && n_carry >= 0 && n_new >= 0 && (long long)n_carry + n_new > 0, "stream_splice_rows: %d rows x channels, carry %d, new %d",
               rows_channels, n_carry, n_new);
  EBEN_REQUIRE(channels > 0 && rows_channels % channels == 0, "stream_splice_rows: %d rows x channels is no multiple of %d channels", rows_channels, channels);
  const int slots = rows_channels / channels;
  EBEN_REQUIRE(slots <= EBEN_STREAM_MAX_SLOTS, "stream_splice_rows: %d slots, at most %d", slots, EBEN_STREAM_MAX_SLOTS);
  SlotMask mask = {{0ull, 0ull, 0ull, 0ull}};
  int n_active = 0;
  for (int q = 0; q < (slots + 63) / 64; ++q) {
    mask.w[q] = active[q];
    const int bits_here = slots - 64 * q;
    EBEN_REQUIRE(bits_here >= 64 || (mask.w[q] >> bits_here) == 0ull, "stream_splice_rows: an active bit at or above the %d slots", slots);
    n_active += __builtin_popcountll(mask.w[q]);
  }
  EBEN_REQUIRE(dst_pitch > 0 && (long long)n_carry + n_new <= dst_pitch, "stream_splice_rows: carry %d + new %d past dst's pitch %d", n_carry, n_new,
               dst_pitch);
  EBEN_REQUIRE(n_carry == 0 || prev, "stream_splice_rows: null prev with a carry of %d", n_carry);
  EBEN_REQUIRE(n_new == 0 || src, "stream_splice_rows: null src with %d new samples", n_new);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(src) |
                         reinterpret_cast<uintptr_t>(add) | reinterpret_cast<uintptr_t>(idle);
  EBEN_REQUIRE((bits & 3) == 0, "stream_splice_rows: misaligned pointer");
  if (n_carry > 0)
    EBEN_REQUIRE(prev_pitch > 0 && prev_off >= 0 && (long long)prev_off + n_carry <= prev_pitch,
                 "stream_splice_rows: prev offset %d + carry %d past its pitch %d", prev_off, n_carry, prev_pitch);
  if (n_new > 0) {
    EBEN_REQUIRE(src_pitch > 0 && src_off >= 0 && (long long)src_off + n_new <= src_pitch, "stream_splice_rows: src offset %d + new %d past its pitch %d",
                 src_off, n_new, src_pitch);
    if (add)
      EBEN_REQUIRE(add_pitch > 0 && add_off >= 0 && (long long)add_off + n_new <= add_pitch, "stream_splice_rows: add offset %d + new %d past its pitch %d",
                   add_off, n_new, add_pitch);
  }
  if (idle)
    EBEN_REQUIRE(idle_pitch > 0 && (long long)n_carry + n_new <= idle_pitch, "stream_splice_rows: carry %d + new %d past idle's pitch %d", n_carry, n_new,
                 idle_pitch);
  // extents: a compact tensor has one row per active slot
  const long long rc = rows_channels, arc = (long long)n_active * channels;
  const long long dst_n = (dst_compact ? arc : rc) * dst_pitch, in_rows = src_compact ? arc : rc;
  if (n_carry > 0) EBEN_REQUIRE(!overlaps(dst, dst_n, prev, rc * prev_pitch), "stream_splice_rows: dst overlaps prev");
  if (n_new > 0) {
    EBEN_REQUIRE(!overlaps(dst, dst_n, src, in_rows * src_pitch), "stream_splice_rows: dst overlaps src");
    if (add) EBEN_REQUIRE(!overlaps(dst, dst_n, add, in_rows * add_pitch), "stream_splice_rows: dst overlaps add");
  }
  if (idle) EBEN_REQUIRE(!overlaps(dst, dst_n, idle, rc * idle_pitch), "stream_splice_rows: dst overlaps idle");
  if (n_active == 0 && (!idle || dst_compact)) return EBEN_OK;   // nothing to write
  const long long total = rc * ((long long)n_carry + n_new);
  const long long blocks = (total + 255) / 256;
  EBEN_REQUIRE(blocks <= 0x7fffffffLL, "stream_splice_rows: grid of %lld blocks", blocks);
  hipLaunchKernelGGL(stream_splice_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dst, dst_pitch, prev, prev_pitch, prev_off,
                     n_carry, src, src_pitch, src_off, n_new, add, add_pitch, add_off, idle, idle_pitch, channels, mask, src_compact ? 1 : 0,
                     dst_compact ? 1 : 0, total);
  EBEN_CHECK_LAUNCH("stream_splice_rows_kernel");
  return EBEN_OK;
}

extern "C" int eben_copy_segments(const EbenCopySegment* segments, int count, void* stream) {
  EBEN_REQUIRE(count >= 0 && count <= EBEN_COPY_MAX_SEGMENTS, "copy_segments: %d segments, at most %d", count, EBEN_COPY_MAX_SEGMENTS);
  if (count == 0) return EBEN_OK;
  EBEN_REQUIRE(segments, "copy_segments: null segment table");
  SegmentTable t;
  long long longest = 0;
  for (int i = 0; i < count; ++i) {
    const EbenCopySegment& s = segments[i];
    EBEN_REQUIRE(s.dst && s.src, "copy_segments: null pointer in segment %d", i);
    EBEN_REQUIRE(((reinterpret_cast<uintptr_t>(s.dst) | reinterpret_cast<uintptr_t>(s.src)) & 3) == 0, "copy_segments: misaligned pointer in segment %d", i);
    EBEN_REQUIRE(s.floats >= 0, "copy_segments: segment %d counts %lld floats", i, s.floats);
    t.s[i] = s;
    longest = s.floats > longest ? s.floats : longest;
  }
  for (int i = 0; i < count; ++i)
    for (int j = 0; j < count; ++j) {
      EBEN_REQUIRE(!overlaps(t.s[i].dst, t.s[i].floats, t.s[j].src, t.s[j].floats), "copy_segments: dst of segment %d overlaps src of segment %d", i, j);
      EBEN_REQUIRE(i >= j || !overlaps(t.s[i].dst, t.s[i].floats, t.s[j].dst, t.s[j].floats), "copy_segments: dst of segment %d overlaps dst of segment %d", i, j);
    }
  if (longest == 0) return EBEN_OK;
  for (int i = count; i < EBEN_COPY_MAX_SEGMENTS; ++i) t.s[i] = EbenCopySegment{nullptr, nullptr, 0};
  long long bx = (longest + 255) / 256;
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(copy_segments_kernel, dim3((unsigned)bx, (unsigned)count), dim3(256), 0, as_stream(stream), t);
  EBEN_CHECK_LAUNCH("copy_segments_kernel");
  return EBEN_OK;
}
