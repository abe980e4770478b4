// Streaming inference: a layer's input for this push, assembled from the previous push's buffer and the producer's fresh output.
//
//   dst[rc, j]           = prev[rc, prev_off + j]                         j < n_carry
//   dst[rc, n_carry + j] = src[rc, src_off + j] (+ add[rc, add_off + j])  j < n_new
//
// rc runs over rows x channels of fp32 [row][C][L] tensors, each with its own row pitch; offsets and counts are arbitrary (scalar
// loads and stores: nothing assumes a 16-byte grid).  dst never aliases a source -- the carry is usually longer than the new part,
// so a shift in place would race; the caller ping-pongs two buffers.  The entry checks every range against its pitch and the four
// extents against each other before it launches: a bad call fails on the host and writes nothing.
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
