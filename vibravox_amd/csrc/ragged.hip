// Ragged batches: rows of different lengths in one (rows, channels, l_buf) buffer.
//
// A conv kernel applies its edge rule (reflect, zero, or the end of a transposed conv) at the end of the BUFFER.  A row that ends at
// len[r] < l_buf gets its own batch-1 result on [0, l_out) when, in front of each layer, the `count` samples behind its end hold what
// the row's own edge rule would have supplied:
//
//   eben_edge_fill   EBEN_FILL_ZERO    x[r, c, len + j] = 0                     j < count
//                    EBEN_FILL_MIRROR  x[r, c, len + j] = x[r, c, len - 2 - j]  j < count   (ReflectionPad1d's index mapping)
//   eben_edge_zero   x[r, c, len + j] = 0 for every j < l_buf - len: the whole slack, for tensors that leave the library
//
// One launch serves every (row, channel) of a tensor; the row lengths come from a device table, so nothing but the launch happens on
// the host.  The kernels check every row themselves -- a row with len == l_buf has no slack and is left alone, a row whose fill would
// leave the buffer or mirror from in front of the row is skipped -- so a bad table cannot make them write out of bounds.
#include "common.h"

namespace eben {
namespace {

// thread = (row * channels + channel, j): `count` is 1 .. 9 on the generator's layers, so consecutive threads write runs of that length
__global__ __launch_bounds__(256) void edge_fill_kernel(float* __restrict__ x, const int* __restrict__ lens, int channels, int l_buf, int mirror,
                                                        int count, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long rc = idx / count;
  const int j = (int)(idx - rc * count);
  const long long len = lens[rc / channels];
  if (len < 0 || len >= l_buf || len + count > l_buf) return;   // no slack, or the fill does not fit
  if (mirror && count > len - 1) return;                      // the mirror image would start in front of the row
  float* row = x + rc * l_buf;
  row[len + j] = mirror ? row[len - 2 - j] : 0.f;
}

// block = 256 consecutive positions of one (row, channel); blocks in front of the row's end leave at once
__global__ __launch_bounds__(256) void edge_zero_kernel(float* __restrict__ x, const int* __restrict__ lens, int channels, int l_buf, int chunks) {
  const long long rc = blockIdx.x / chunks;
  const long long p0 = (long long)(blockIdx.x - rc * chunks) * 256;
  const long long len = lens[rc / channels];
  if (len < 0 || p0 + 256 <= len) return;
  const long long p = p0 + threadIdx.x;
  if (p >= len && p < l_buf) x[rc * l_buf + p] = 0.f;
}

int check_table_args(const void* x, const int32_t* lens, int rows, int channels, int l_buf, const char* what) {
  EBEN_REQUIRE(x && lens, "%s: null pointer", what);
  EBEN_REQUIRE((reinterpret_cast<size_t>(x) & 3) == 0 && (reinterpret_cast<size_t>(lens) & 3) == 0, "%s: misaligned pointer", what);
  EBEN_REQUIRE(rows > 0 && channels > 0 && l_buf > 0, "%s: rows %d, channels %d, l_buf %d", what, rows, channels, l_buf);
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_edge_fill(float* x, const int32_t* lens, int rows, int channels, int l_buf, int mode, int count, void* stream) {
  if (int rc = check_table_args(x, lens, rows, channels, l_buf, "edge_fill")) return rc;
  EBEN_REQUIRE(mode == EBEN_FILL_ZERO || mode == EBEN_FILL_MIRROR, "edge_fill: mode %d", mode);
  EBEN_REQUIRE(count >= 1 && count < l_buf, "edge_fill: count %d on a buffer of %d samples", count, l_buf);
  const long long total = (long long)rows * channels * count;
  const long long blocks = (total + 255) / 256;
  EBEN_REQUIRE(blocks <= 0x7fffffffLL, "edge_fill: grid of %lld blocks", blocks);
  hipLaunchKernelGGL(edge_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, lens, channels, l_buf,
                     mode == EBEN_FILL_MIRROR ? 1 : 0, count, total);
  EBEN_CHECK_LAUNCH("edge_fill_kernel");
  return EBEN_OK;
}

extern "C" int eben_edge_zero(float* x, const int32_t* lens, int rows, int channels, int l_buf, void* stream) {
  if (int rc = check_table_args(x, lens, rows, channels, l_buf, "edge_zero")) return rc;
  const int chunks = ceil_div(l_buf, 256);
  const long long blocks = (long long)rows * channels * chunks;
  EBEN_REQUIRE(blocks <= 0x7fffffffLL, "edge_zero: grid of %lld blocks", blocks);
  hipLaunchKernelGGL(edge_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, lens, channels, l_buf, chunks);
  EBEN_CHECK_LAUNCH("edge_zero_kernel");
  return EBEN_OK;
}
