// Recordings to resident clips: the `data` chunks of many WAVE files, uploaded as they lie on disk, become rows of float32 in one launch.
//
// A row is one channel of one file: EbenPcmRow names where the file's interleaved frames start in the byte buffer (16-byte aligned),
// how many frames there are, how many channels a frame has, which one to take, and the sample format.  Each conversion is exact:
//
//   PCM16  x * 2^-15        PCM24  sign-extended x * 2^-23        PCM32  float(x) * 2^-31, float(x) rounded to nearest once        FLOAT32  the bits
//
// Two kernels share the row table and the two output forms (padded rows with a length table as eben_resample_ragged takes and writes
// them, or flat: row r's samples at out[out_offsets[r]], nothing else touched):
//
//   pcm_decode_kernel   a block owns PCM_TILE consecutive samples of one row.  Mono PCM16 -- what a Vibravox sensor file is -- takes one
//                       16-byte load per lane (8 samples), converts into LDS and stores from there, so loads and stores are both
//                       coalesced whatever the output's alignment; every other row reads its samples one by one with stride `channels`.
//   pcm_rate_kernel     rate.hip's tile (rate_tile.h: same tile constants, same ascending-j fmaf chain, same stores) with its window staged
//                       by the converting load: row r's outputs are bit for bit eben_resample_ragged's on the decoded row.
//
// The host validates its own copy of the table before anything is launched; the kernels read the uploaded copy and treat a row whose
// numbers would reach outside the byte buffer or the output as empty, so a stale upload cannot make them read or write out of bounds.
#include "rate_tile.h"

namespace eben {
namespace {

constexpr int PCM_THREADS = 256;
constexpr int PCM_PER_THREAD = 8;                        // one 16-byte load of PCM16
constexpr int PCM_TILE = PCM_THREADS * PCM_PER_THREAD;   // samples per block
constexpr int PCM_MAX_CHANNELS = 65535;

struct PcmArgs {
  const unsigned char* data;
  long long data_bytes;
  const EbenPcmRow* rows;       // device copy of the table
  const long long* out_off;     // flat form: per-row offset into out, in floats; null: rows of `extent` floats
  float* out;
  int* out_lens;                // nullable in the flat form
  long long extent;             // padded: the pitch; flat: floats of the whole store
};

__host__ __device__ inline int pcm_bytes(int format) { return format == EBEN_PCM_S16 ? 2 : format == EBEN_PCM_S24 ? 3 : 4; }

// the row's descriptor with `frames` set to 0 when its numbers do not fit the byte buffer
__device__ __forceinline__ EbenPcmRow pcm_row(const PcmArgs& p, int r) {
  EbenPcmRow d = p.rows[r];
  const bool ok = d.format >= EBEN_PCM_S16 && d.format <= EBEN_PCM_F32 && d.channels >= 1 && d.channels <= PCM_MAX_CHANNELS && d.channel >= 0 &&
                  d.channel < d.channels && d.frames >= 0 && d.frames <= RATE_MAX_SAMPLES && d.byte_offset >= 0 && (d.byte_offset & 15) == 0 &&
                  d.byte_offset + (long long)d.frames * d.channels * pcm_bytes(d.format) <= p.data_bytes;
  if (!ok) d.frames = 0;
  return d;
}

__device__ __forceinline__ float pcm16(int v) { return (float)v * 0x1p-15f; }

// frame i of the row, its selected channel
__device__ __forceinline__ float pcm_sample(const unsigned char* base, int format, int channels, int channel, int i) {
  const long long e = (long long)i * channels + channel;
  if (format == EBEN_PCM_S16) return pcm16(*reinterpret_cast<const short*>(base + 2 * e));
  if (format == EBEN_PCM_S24) {
    const unsigned char* b = base + 3 * e;
    const int v = (int)b[0] | ((int)b[1] << 8) | ((int)(signed char)b[2] << 16);
    return (float)v * 0x1p-23f;
  }
  if (format == EBEN_PCM_S32) return (float)*reinterpret_cast<const int*>(base + 4 * e) * 0x1p-31f;
  return *reinterpret_cast<const float*>(base + 4 * e);
}

// 8 PCM16 samples of one 16-byte load, in memory order
__device__ __forceinline__ void pcm16x8(const uint4 q, float4* lo, float4* hi) {
  lo->x = pcm16((short)(q.x & 0xffffu));
  lo->y = pcm16((short)(q.x >> 16));
  lo->z = pcm16((short)(q.y & 0xffffu));
  lo->w = pcm16((short)(q.y >> 16));
  hi->x = pcm16((short)(q.z & 0xffffu));
  hi->y = pcm16((short)(q.z >> 16));
  hi->z = pcm16((short)(q.w & 0xffffu));
  hi->w = pcm16((short)(q.w >> 16));
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_decode_kernel(PcmArgs p) {
  __shared__ __attribute__((aligned(16))) float buf[PCM_TILE];
  const int r = blockIdx.y, t = threadIdx.x;
  const EbenPcmRow d = pcm_row(p, r);
  int frames = d.frames;
  float* o;
  int fill_to;
  if (p.out_off) {
    const long long off = p.out_off[r];
    if (off < 0 || off + frames > p.extent) frames = 0;
    o = p.out + off;
    fill_to = frames;
  } else {
    if (frames > p.extent) frames = 0;
    o = p.out + (long long)r * p.extent;
    fill_to = (int)p.extent;
  }
  if (blockIdx.x == 0 && t == 0 && p.out_lens) p.out_lens[r] = frames;
  const long long n0l = (long long)blockIdx.x * PCM_TILE;
  if (n0l >= fill_to) return;   // the whole block: nothing of this row lies here
  const int n0 = (int)n0l;
  const unsigned char* base = p.data + d.byte_offset;
  if (d.format == EBEN_PCM_S16 && d.channels == 1 && n0 < frames) {
    const int i = n0 + PCM_PER_THREAD * t;
    float4 lo, hi;
    if (i + PCM_PER_THREAD <= frames) {
      pcm16x8(*reinterpret_cast<const uint4*>(base + 2 * (long long)i), &lo, &hi);   // 16-byte aligned: the chunk is, and i is a multiple of 8
    } else {
      float v[PCM_PER_THREAD];
#pragma unroll
      for (int k = 0; k < PCM_PER_THREAD; ++k) v[k] = i + k < frames ? pcm16(*reinterpret_cast<const short*>(base + 2 * (long long)(i + k))) : 0.f;
      lo = make_float4(v[0], v[1], v[2], v[3]);
      hi = make_float4(v[4], v[5], v[6], v[7]);
    }
    *reinterpret_cast<float4*>(buf + PCM_PER_THREAD * t) = lo;
    *reinterpret_cast<float4*>(buf + PCM_PER_THREAD * t + 4) = hi;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PCM_PER_THREAD; ++k) {
      const int s = t + PCM_THREADS * k;
      if (n0 + s < fill_to) o[n0 + s] = buf[s];   // behind the row's end the staged value is the zero of the padding
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < PCM_PER_THREAD; ++k) {
    const long long n = n0l + t + PCM_THREADS * k;
    if (n < frames)
      o[n] = pcm_sample(base, d.format, d.channels, d.channel, (int)n);
    else if (n < fill_to)
      o[n] = 0.f;
  }
}

// rate_tile.h's window from PCM frames: the indices [w0, w0 + wlen) of the row's selected channel, zero outside [0, len).  Mono PCM16
// takes 16-byte loads over the part of the window that is aligned in memory and lies inside the row (8 samples = two 16-byte LDS slots,
// the LDS copy shifted so that they land on slots); every other row is read sample by sample.
struct PcmStage {
  const unsigned char* base;
  int format, channels, channel;
  __device__ __forceinline__ float* operator()(int w0, int wlen, int len, float* win_raw) const {
    const int t = threadIdx.x;
    if (!(format == EBEN_PCM_S16 && channels == 1)) {
      for (int s = t; s < wlen; s += RATE_THREADS) {
        const int i = w0 + s;
        win_raw[s] = (i >= 0 && i < len) ? pcm_sample(base, format, channels, channel, i) : 0.f;
      }
      return win_raw;
    }
    const short* xr = reinterpret_cast<const short*>(base);
    const int head = (int)((0u - (unsigned)w0) & 7u);   // samples in front of the first 16-byte boundary of memory
    float* win = win_raw + ((4 - (head & 3)) & 3);      // so that win + head is a 16-byte LDS slot
    if (t < head && t < wlen) {
      const int i = w0 + t;
      win[t] = (i >= 0 && i < len) ? pcm16(xr[i]) : 0.f;
    }
    const int nvec = wlen > head ? (wlen - head) >> 3 : 0;
    for (int v = t; v < nvec; v += RATE_THREADS) {
      const int s = head + 8 * v, i = w0 + s;
      float4 lo, hi;
      if (i >= 0 && i + 7 < len) {
        pcm16x8(*reinterpret_cast<const uint4*>(xr + i), &lo, &hi);
      } else {
        float q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = (i + k >= 0 && i + k < len) ? pcm16(xr[i + k]) : 0.f;
        lo = make_float4(q[0], q[1], q[2], q[3]);
        hi = make_float4(q[4], q[5], q[6], q[7]);
      }
      *reinterpret_cast<float4*>(win + s) = lo;
      *reinterpret_cast<float4*>(win + s + 4) = hi;
    }
    {
      const int s = head + 8 * nvec + t;   // at most 7 left
      if (t < 8 && s < wlen) {
        const int i = w0 + s;
        win[s] = (i >= 0 && i < len) ? pcm16(xr[i]) : 0.f;
      }
    }
    return win;
  }
};

template <int TABLE>
__global__ __launch_bounds__(RATE_THREADS) void pcm_rate_kernel(RateArgs a, PcmArgs p) {
  __shared__ __attribute__((aligned(16))) float win_raw[RATE_WINDOW_FLOATS + 4];
  __shared__ float tab[TABLE ? RATE_TABLE_FLOATS : 1];
  const int r = blockIdx.y;
  const EbenPcmRow d = pcm_row(p, r);
  int len = d.frames;
  long long n_out = ((long long)a.nw * len + a.orig - 1) / a.orig;
  float* o;
  if (p.out_off) {
    const long long off = p.out_off[r];
    if (off < 0 || off + n_out > p.extent) len = 0, n_out = 0;
    o = p.out + off;
  } else {
    if (n_out > p.extent) len = 0, n_out = 0;
    o = p.out + (long long)r * p.extent;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && p.out_lens) p.out_lens[r] = (int)n_out;
  rate_tile_staged<TABLE>(a, PcmStage{p.data + d.byte_offset, d.format, d.channels, d.channel}, o, len, (int)n_out, blockIdx.x, win_raw, tab);
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// The host's copy of the table against the byte buffer and the output; *longest = the most outputs any row has (ceil(nw * frames / orig)).
int check_rows(const char* what, const void* data, long long data_bytes, const EbenPcmRow* rows_host, const EbenPcmRow* rows_dev,
               const long long* off_host, const long long* off_dev, const float* out, const int32_t* out_lens, int rows, long long extent, int orig, int nw,
               long long* longest) {
  EBEN_REQUIRE(data && rows_host && rows_dev && out, "%s: null pointer", what);
  EBEN_REQUIRE((off_host == nullptr) == (off_dev == nullptr), "%s: the output offsets need their host and their device copy, or neither", what);
  EBEN_REQUIRE(off_host || out_lens, "%s: null pointer (padded rows need out_lens)", what);
  EBEN_REQUIRE(aligned_to(data, 16) && aligned_to(rows_host, 8) && aligned_to(rows_dev, 8) && aligned_to(off_host, 8) && aligned_to(off_dev, 8) &&
                   aligned4(out) && aligned4(out_lens),
               "%s: misaligned pointer (data to 16 bytes, tables to 8, out and out_lens to 4)", what);
  EBEN_REQUIRE(rows > 0 && rows <= 65535, "%s: %d rows (1 ... 65535)", what, rows);
  EBEN_REQUIRE(data_bytes >= 0, "%s: a byte buffer of %lld bytes", what, data_bytes);
  if (off_host)
    EBEN_REQUIRE(extent >= 0, "%s: a store of %lld floats", what, extent);
  else
    EBEN_REQUIRE(extent > 0 && extent <= RATE_MAX_SAMPLES, "%s: a pitch of %lld floats (1 ... %d)", what, extent, RATE_MAX_SAMPLES);
  long long most = 0, floor_off = 0;
  for (int r = 0; r < rows; ++r) {
    const EbenPcmRow& d = rows_host[r];
    EBEN_REQUIRE(d.format >= EBEN_PCM_S16 && d.format <= EBEN_PCM_F32, "%s: row %d has the unknown format %d", what, r, d.format);
    EBEN_REQUIRE(d.channels >= 1 && d.channels <= PCM_MAX_CHANNELS, "%s: row %d has %d channels (1 ... %d)", what, r, d.channels, PCM_MAX_CHANNELS);
    EBEN_REQUIRE(d.channel >= 0 && d.channel < d.channels, "%s: row %d takes channel %d of %d", what, r, d.channel, d.channels);
    EBEN_REQUIRE(d.frames >= 0 && d.frames <= RATE_MAX_SAMPLES, "%s: row %d has %d frames (0 ... %d)", what, r, d.frames, RATE_MAX_SAMPLES);
    EBEN_REQUIRE(d.byte_offset >= 0 && (d.byte_offset & 15) == 0, "%s: row %d starts at byte %lld, not a multiple of 16", what, r, d.byte_offset);
    const long long bytes = (long long)d.frames * d.channels * pcm_bytes(d.format);
    EBEN_REQUIRE(d.byte_offset + bytes <= data_bytes, "%s: row %d holds bytes [%lld, %lld) of a buffer of %lld", what, r, d.byte_offset,
                 d.byte_offset + bytes, data_bytes);
    const long long n = ((long long)nw * d.frames + orig - 1) / orig;
    EBEN_REQUIRE(n <= RATE_MAX_SAMPLES, "%s: row %d would have %lld samples (at most %d)", what, r, n, RATE_MAX_SAMPLES);
    if (off_host) {
      const long long off = off_host[r];
      EBEN_REQUIRE(off >= floor_off && off + n <= extent, "%s: row %d writes [%lld, %lld) of a store of %lld floats whose first free float is %lld", what, r, off,
                   off + n, extent, floor_off);
      floor_off = off + n;
    } else {
      EBEN_REQUIRE(n <= extent, "%s: the pitch %lld is too small for row %d of %lld samples", what, extent, r, n);
    }
    most = n > most ? n : most;
  }
  *longest = most;
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_pcm_decode_ragged(const void* data, long long data_bytes, const EbenPcmRow* rows_host, const EbenPcmRow* rows_dev,
                                      const long long* out_offsets_host, const long long* out_offsets_dev, float* out, int32_t* out_lens, int rows,
                                      long long out_extent, void* stream) {
  long long longest = 0;
  if (int rc = check_rows("pcm_decode_ragged", data, data_bytes, rows_host, rows_dev, out_offsets_host, out_offsets_dev, out, out_lens, rows, out_extent, 1,
                          1, &longest))
    return rc;
  const long long places = out_offsets_host ? longest : out_extent;
  if (places == 0 && !out_lens) return EBEN_OK;   // flat, every row empty, no table to fill
  const long long tiles = places == 0 ? 1 : (places + PCM_TILE - 1) / PCM_TILE;
  const PcmArgs p{static_cast<const unsigned char*>(data), data_bytes, rows_dev, out_offsets_dev, out, out_lens, out_extent};
  hipLaunchKernelGGL(pcm_decode_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(PCM_THREADS), 0, as_stream(stream), p);
  EBEN_CHECK_LAUNCH("pcm_decode_kernel");
  return EBEN_OK;
}

extern "C" int eben_pcm_resample_ragged(const void* data, long long data_bytes, const EbenPcmRow* rows_host, const EbenPcmRow* rows_dev,
                                        const float* kernels, const long long* out_offsets_host, const long long* out_offsets_dev, float* out,
                                        int32_t* out_lens, int rows, long long out_extent, int orig, int nw, int width, void* stream) {
  EBEN_REQUIRE(kernels, "pcm_resample_ragged: null pointer");
  EBEN_REQUIRE(aligned4(kernels), "pcm_resample_ragged: misaligned pointer");
  int taps = 0, tq = 0;
  if (int rc = check_ratio("pcm_resample_ragged", orig, nw, width, &taps, &tq)) return rc;
  long long longest = 0;
  if (int rc = check_rows("pcm_resample_ragged", data, data_bytes, rows_host, rows_dev, out_offsets_host, out_offsets_dev, out, out_lens, rows, out_extent,
                          orig, nw, &longest))
    return rc;
  const long long places = out_offsets_host ? longest : out_extent;
  if (places == 0 && !out_lens) return EBEN_OK;
  const long long to = (long long)tq * nw, tiles = places == 0 ? 1 : (places + to - 1) / to;
  EBEN_REQUIRE(tiles <= 0x7fffffffLL, "pcm_resample_ragged: grid of %lld tiles", tiles);
  // lens / out_lens / the pitches of RateArgs stay unused: the row's numbers come from its descriptor
  const RateArgs a{nullptr, kernels, nullptr, nullptr, nullptr, 0, 0, 0, orig, nw, taps, tq, 0, -width, 0, 0, out_offsets_host ? 0 : (int)out_extent};
  const PcmArgs p{static_cast<const unsigned char*>(data), data_bytes, rows_dev, out_offsets_dev, out, out_lens, out_extent};
  const dim3 grid((unsigned)tiles, (unsigned)rows), block(RATE_THREADS);
  switch (rate_table_route(nw, taps)) {
    case 0: hipLaunchKernelGGL(pcm_rate_kernel<0>, grid, block, 0, as_stream(stream), a, p); break;
    case 2: hipLaunchKernelGGL(pcm_rate_kernel<2>, grid, block, 0, as_stream(stream), a, p); break;
    default: hipLaunchKernelGGL(pcm_rate_kernel<1>, grid, block, 0, as_stream(stream), a, p); break;
  }
  EBEN_CHECK_LAUNCH("pcm_rate_kernel");
  return EBEN_OK;
}
