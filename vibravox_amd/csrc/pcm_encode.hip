// Rows of float32 to the bytes of WAVE files: corpus.hip's decoder the other way round.  Many rows, each anywhere in one float buffer
// (a row of a padded batch buffer at r * pitch, a clip inside a flat store), become the mono little-endian `data` bytes of many files in
// one flat byte image, in one launch.  With b the bit depth and v = rint(x * 2^(b-1)), half to even in float32:
//
//   PCM16 / PCM24 / PCM32  v clamped to [-2^(b-1), 2^(b-1) - 1], NaN stores 0        FLOAT32  the bits of x
//
// and a sample counts as clipped when v >= 2^(b-1), v < -2^(b-1) or x is a NaN; the per-row counts are integer sums (LDS and global
// integer atomics), the same on every run.
//
//   pcm_encode_kernel   a block owns ENC_TILE consecutive samples of one row.  PCM16 -- what a Vibravox sensor file is -- reads its floats
//                       one per lane (coalesced wherever the row starts on the 4-byte grid), converts into LDS and stores 16 bytes (8
//                       samples) per lane from there: the image offset is a multiple of 16, so every full vector is aligned; the last
//                       partial vector of a row goes out sample by sample.  The other formats store sample by sample.
//                       pcm_encode_kernel<true> (eben_pcm_encode_ragged_gain) is the same body with every sample read as x * gains[row],
//                       rounded to float32, in front of the conversion: a loudness-normalised export without a scaled copy of the rows.
//
// Only the rows' own bytes are written.  The host validates its own copy of the table before anything is launched; the kernel reads the
// uploaded copy and treats a row whose numbers would reach outside the source or the image as empty.
#include <algorithm>
#include <vector>

#include "common.h"

namespace eben {
namespace {

constexpr int ENC_THREADS = 256;
constexpr int ENC_PER_THREAD = 8;                        // one 16-byte store of PCM16
constexpr int ENC_TILE = ENC_THREADS * ENC_PER_THREAD;   // samples per block
constexpr int ENC_MAX_SAMPLES = 0x7fff0000;              // per row: every index plus a tile stays inside int32

struct EncArgs {
  const float* src;
  long long src_floats;
  const EbenPcmEncRow* rows;   // device copy of the table
  unsigned char* image;
  long long image_bytes;
  int* clipped;
  const float* gains;   // pcm_encode_kernel<true> only: one factor per row
};

__host__ __device__ inline int enc_bytes(int format) { return format == EBEN_PCM_S16 ? 2 : format == EBEN_PCM_S24 ? 3 : 4; }

// the row's descriptor with `samples` set to 0 when its numbers do not fit the source or the image
__device__ __forceinline__ EbenPcmEncRow enc_row(const EncArgs& p, int r) {
  EbenPcmEncRow d = p.rows[r];
  const bool ok = d.format >= EBEN_PCM_S16 && d.format <= EBEN_PCM_F32 && d.samples >= 0 && d.samples <= ENC_MAX_SAMPLES && d.src_offset >= 0 &&
                  d.src_offset <= p.src_floats && d.src_offset + d.samples <= p.src_floats && d.byte_offset >= 0 && (d.byte_offset & 15) == 0 &&
                  d.byte_offset <= p.image_bytes && d.byte_offset + (long long)d.samples * enc_bytes(d.format) <= p.image_bytes;
  if (!ok) d.samples = 0;
  return d;
}

// the stored integer of a sample; *clip counts what left the range
template <int BITS>
__device__ __forceinline__ int enc_int(float x, int* clip) {
  constexpr float scale = (float)(1ll << (BITS - 1));
  constexpr int hi = (int)((1ll << (BITS - 1)) - 1), lo = (int)(-(1ll << (BITS - 1)));
  const float v = rintf(x * scale);   // an exact power-of-two scaling, then round half to even
  if (x != x) {
    ++*clip;
    return 0;
  }
  if (v >= scale) {
    ++*clip;
    return hi;
  }
  if (v < -scale) {
    ++*clip;
    return lo;
  }
  return (int)v;
}

template <bool GAIN>
__global__ __launch_bounds__(ENC_THREADS) void pcm_encode_kernel(EncArgs p) {
  __shared__ __attribute__((aligned(16))) short buf[ENC_TILE];
  __shared__ int block_clip;
  const int r = blockIdx.y, t = threadIdx.x;
  const EbenPcmEncRow d = enc_row(p, r);
  const int samples = d.samples;
  const long long n0l = (long long)blockIdx.x * ENC_TILE;
  if (n0l >= samples) return;   // the whole block: nothing of this row lies here
  const int n0 = (int)n0l;
  if (t == 0) block_clip = 0;
  __syncthreads();
  const float* x = p.src + d.src_offset;
  unsigned char* o = p.image + d.byte_offset;
  int clip = 0;
  const float g = GAIN ? p.gains[r] : 1.f;
  auto sample = [&](long long n) { return GAIN ? x[n] * g : x[n]; };   // the product rounds to float32 before anything else sees it
  if (d.format == EBEN_PCM_S16) {
#pragma unroll
    for (int k = 0; k < ENC_PER_THREAD; ++k) {
      const int s = t + ENC_THREADS * k;
      if (n0 + s < samples) buf[s] = (short)enc_int<16>(sample(n0 + s), &clip);
    }
    if (clip) atomicAdd(&block_clip, clip);
    __syncthreads();
    const int s = ENC_PER_THREAD * t, i = n0 + s;
    if (i + ENC_PER_THREAD <= samples) {
      *reinterpret_cast<uint4*>(o + 2 * (long long)i) = *reinterpret_cast<const uint4*>(buf + s);   // 16-byte aligned: the row is, i is a multiple of 8
    } else {
      for (int k = 0; i + k < samples; ++k) *reinterpret_cast<short*>(o + 2 * (long long)(i + k)) = buf[s + k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < ENC_PER_THREAD; ++k) {
      const long long n = n0l + t + ENC_THREADS * k;
      if (n >= samples) continue;
      if (d.format == EBEN_PCM_S24) {
        const int v = enc_int<24>(sample(n), &clip);
        unsigned char* b = o + 3 * n;
        b[0] = (unsigned char)v;
        b[1] = (unsigned char)(v >> 8);
        b[2] = (unsigned char)(v >> 16);
      } else if (d.format == EBEN_PCM_S32) {
        *reinterpret_cast<int*>(o + 4 * n) = enc_int<32>(sample(n), &clip);
      } else if (GAIN) {
        *reinterpret_cast<float*>(o + 4 * n) = sample(n);
      } else {
        *reinterpret_cast<unsigned*>(o + 4 * n) = reinterpret_cast<const unsigned*>(x)[n];
      }
    }
    if (clip) atomicAdd(&block_clip, clip);
    __syncthreads();
  }
  if (t == 0 && block_clip) atomicAdd(p.clipped + r, block_clip);
}

inline bool enc_aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

struct EncSpan {
  long long lo, hi;
  int row;
};

// what the two entry points share: `gains` null is eben_pcm_encode_ragged
int enc_launch(const char* what, const float* src, long long src_floats, const EbenPcmEncRow* rows_host, const EbenPcmEncRow* rows_dev, void* image,
               long long image_bytes, int32_t* clipped, const float* gains, int rows, void* stream) {
  EBEN_REQUIRE(src && rows_host && rows_dev && image && clipped, "%s: null pointer", what);
  EBEN_REQUIRE(enc_aligned(image, 16) && enc_aligned(rows_host, 8) && enc_aligned(rows_dev, 8) && enc_aligned(src, 4) && enc_aligned(clipped, 4),
               "%s: misaligned pointer (image to 16 bytes, tables to 8, src and clipped to 4)", what);
  EBEN_REQUIRE(rows > 0 && rows <= 65535, "%s: %d rows (1 ... 65535)", what, rows);
  EBEN_REQUIRE(src_floats >= 0, "%s: a source of %lld floats", what, src_floats);
  EBEN_REQUIRE(image_bytes >= 0, "%s: an image of %lld bytes", what, image_bytes);
  int longest = 0;
  std::vector<EncSpan> spans;
  spans.reserve(rows);
  for (int r = 0; r < rows; ++r) {
    const EbenPcmEncRow& d = rows_host[r];
    EBEN_REQUIRE(d.format >= EBEN_PCM_S16 && d.format <= EBEN_PCM_F32, "%s: row %d has the unknown format %d", what, r, d.format);
    EBEN_REQUIRE(d.samples >= 0 && d.samples <= ENC_MAX_SAMPLES, "%s: row %d has %d samples (0 ... %d)", what, r, d.samples, ENC_MAX_SAMPLES);
    EBEN_REQUIRE(d.src_offset >= 0 && d.src_offset <= src_floats && d.src_offset + d.samples <= src_floats,
                 "%s: row %d reads the floats [%lld, %lld) of a source of %lld", what, r, d.src_offset, d.src_offset + d.samples, src_floats);
    EBEN_REQUIRE(d.byte_offset >= 0 && (d.byte_offset & 15) == 0, "%s: row %d starts at byte %lld, not a multiple of 16", what, r, d.byte_offset);
    const long long bytes = (long long)d.samples * enc_bytes(d.format);
    EBEN_REQUIRE(d.byte_offset <= image_bytes && d.byte_offset + bytes <= image_bytes, "%s: row %d writes the bytes [%lld, %lld) of an image of %lld", what, r,
                 d.byte_offset, d.byte_offset + bytes, image_bytes);
    if (bytes) spans.push_back(EncSpan{d.byte_offset, d.byte_offset + bytes, r});
    longest = d.samples > longest ? d.samples : longest;
  }
  std::sort(spans.begin(), spans.end(), [](const EncSpan& a, const EncSpan& b) { return a.lo < b.lo; });
  for (size_t k = 1; k < spans.size(); ++k)
    EBEN_REQUIRE(spans[k].lo >= spans[k - 1].hi, "%s: rows %d and %d overlap in the image: bytes [%lld, %lld) and [%lld, %lld)", what, spans[k - 1].row,
                 spans[k].row, spans[k - 1].lo, spans[k - 1].hi, spans[k].lo, spans[k].hi);
  const hipError_t e = hipMemsetAsync(clipped, 0, sizeof(int32_t) * (size_t)rows, as_stream(stream));
  if (e != hipSuccess) return hip_fail(e, "pcm_encode_ragged: zeroing the clipped counts");
  if (longest == 0) return EBEN_OK;   // every row empty
  const int tiles = (longest + ENC_TILE - 1) / ENC_TILE;
  const EncArgs p{src, src_floats, rows_dev, static_cast<unsigned char*>(image), image_bytes, clipped, gains};
  const dim3 grid((unsigned)tiles, (unsigned)rows);
  if (gains) {
    hipLaunchKernelGGL(pcm_encode_kernel<true>, grid, dim3(ENC_THREADS), 0, as_stream(stream), p);
  } else {
    hipLaunchKernelGGL(pcm_encode_kernel<false>, grid, dim3(ENC_THREADS), 0, as_stream(stream), p);
  }
  EBEN_CHECK_LAUNCH("pcm_encode_kernel");
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_pcm_encode_plan(int* out, int n) {
  EBEN_REQUIRE(out && n >= 1, "pcm_encode_plan: needs room for 1 value, got %d at %p", n, (void*)out);
  out[0] = ENC_TILE;
  return EBEN_OK;
}

extern "C" int eben_pcm_encode_ragged(const float* src, long long src_floats, const EbenPcmEncRow* rows_host, const EbenPcmEncRow* rows_dev, void* image,
                                      long long image_bytes, int32_t* clipped, int rows, void* stream) {
  return enc_launch("pcm_encode_ragged", src, src_floats, rows_host, rows_dev, image, image_bytes, clipped, nullptr, rows, stream);
}

extern "C" int eben_pcm_encode_ragged_gain(const float* src, long long src_floats, const EbenPcmEncRow* rows_host, const EbenPcmEncRow* rows_dev,
                                           void* image, long long image_bytes, int32_t* clipped, const float* gains, int rows, void* stream) {
  EBEN_REQUIRE(gains && enc_aligned(gains, 4), "pcm_encode_ragged_gain: a null or misaligned table of gains");
  return enc_launch("pcm_encode_ragged_gain", src, src_floats, rows_host, rows_dev, image, image_bytes, clipped, gains, rows, stream);
}
