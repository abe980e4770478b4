// The resampling tile of rate.hip, with the staging of its input window left to the caller: rate.hip stages float32 rows, corpus.hip
// stages the selected channel of interleaved PCM frames, converted on the way into LDS.  Everything behind the barrier -- the phase
// grid, the ascending-j fmaf chain, the stores and the zero fill -- is one device function, so both give the same bits.
#pragma once
#include "common.h"

namespace eben {
namespace {

constexpr int RATE_THREADS = 256;
constexpr int RATE_PER_THREAD = 4;
constexpr int RATE_TILE_OUT = RATE_THREADS * RATE_PER_THREAD;   // outputs per block at most
constexpr int RATE_WINDOW_FLOATS = 4096;                        // LDS budget of the input window ...
constexpr int RATE_TABLE_FLOATS = 2048;                         // ... and of the table
constexpr int RATE_MAX_SAMPLES = 0x7fff0000;                    // per row: every index plus a tile stays inside int32

struct RateArgs {
  const float* x;          // rows of in_pitch floats
  const float* kernels;    // (nw, taps)
  float* out;              // rows of out_pitch floats
  const int* lens;         // per-row length (ragged) or null: `len` for every row
  int* out_lens;           // ragged: receives ceil(nw * len / orig) per row; else null
  int len, in_pitch, out_pitch;
  int orig, nw, taps, tq;
  int p0, base0;           // phase of output 0 and buffer index of its tap 0
  int first_out, n_out;    // outputs go to out[first_out + n], n < n_out (ragged: n_out per row from its length)
  int fill_to;             // exact zeros to out[first_out + n] for n_out <= n < fill_to (0: none)
};

// Stages the buffer indices [w0, w0 + wlen) of a float32 row of `len` samples, zero outside [0, len): 16-byte loads over the part of the
// window that is aligned in memory and lies inside the row, the LDS copy shifted so that those land on 16-byte LDS slots.  Returns where
// index w0 landed (win_raw: RATE_WINDOW_FLOATS + 4 floats, 16-byte aligned).
struct RateStageF32 {
  const float* xr;
  __device__ __forceinline__ float* operator()(int w0, int wlen, int len, float* win_raw) const {
    const int t = threadIdx.x;
    // floats in front of the first 16-byte boundary of memory; the LDS copy starts (4 - head) & 3 floats in, so that boundary is a slot
    const int head = (int)((0u - (unsigned)(((unsigned long long)reinterpret_cast<uintptr_t>(xr) >> 2) + (unsigned long long)(long long)w0)) & 3u);
    float* win = win_raw + ((4 - head) & 3);
    if (t < head && t < wlen) {
      const int i = w0 + t;
      win[t] = (i >= 0 && i < len) ? xr[i] : 0.f;
    }
    const int nvec = wlen > head ? (wlen - head) >> 2 : 0;
    for (int v = t; v < nvec; v += RATE_THREADS) {
      const int s = head + 4 * v, i = w0 + s;
      float4 q;
      if (i >= 0 && i + 3 < len) {
        q = *reinterpret_cast<const float4*>(xr + i);
      } else {
        q.x = (i >= 0 && i < len) ? xr[i] : 0.f;
        q.y = (i + 1 >= 0 && i + 1 < len) ? xr[i + 1] : 0.f;
        q.z = (i + 2 >= 0 && i + 2 < len) ? xr[i + 2] : 0.f;
        q.w = (i + 3 >= 0 && i + 3 < len) ? xr[i + 3] : 0.f;
      }
      *reinterpret_cast<float4*>(win + s) = q;
    }
    {
      const int s = head + 4 * nvec + t;   // at most 3 left
      if (s >= head && s < wlen) {
        const int i = w0 + s;
        win[s] = (i >= 0 && i < len) ? xr[i] : 0.f;
      }
    }
    return win;
  }
};

// One tile of one row: `stage` hands over the row's window (a row of `len` samples), `o` is where its output 0 goes, `tile` its place
// among the row's tiles; the ratio, p0, base0 and fill_to come from `a`.  `win_raw` (RATE_WINDOW_FLOATS + 4 floats, 16-byte aligned) and
// `tab` are the block's LDS.
// TABLE: 0 = table through L2, 1 = table in LDS, 2 = table in LDS and nw == 1 (one value per tap for all outputs of a thread)
template <int TABLE, class Stage>
__device__ __forceinline__ void rate_tile_staged(const RateArgs& a, const Stage& stage, float* o, int len, int n_out, int tile, float* win_raw,
                                                 float* tab) {
  const int t = threadIdx.x;
  const int orig = a.orig, nw = a.nw, taps = a.taps;
  const int to = a.tq * nw;              // outputs of a tile
  const int g0 = tile * to;              // the tile's first place in the launch's phase grid
  const int n_lo = g0 - a.p0;            // output index of the tile's place 0 (below 0 in the first tile when p0 > 0)
  if (n_lo >= n_out) {                   // nothing to compute: the slack behind the row
    for (int i = 0; i < RATE_PER_THREAD; ++i) {
      const int n = n_lo + t + RATE_THREADS * i;
      if (t + RATE_THREADS * i < to && n < a.fill_to) o[n] = 0.f;
    }
    return;
  }
  // ---- stage the window: buffer indices [w0, w0 + wlen), zero outside [0, len) -----------------------------------------------------
  const int w0 = a.base0 + tile * a.tq * orig;
  const int wlen = a.tq * orig + taps - 1;
  const float* win = stage(w0, wlen, len, win_raw);
  if (TABLE) {
    const int nt = nw * taps;
    for (int s = t; s < nt; s += RATE_THREADS) tab[s] = a.kernels[s];
  }
  __syncthreads();
  // ---- four outputs per thread, RATE_THREADS apart: consecutive lanes consecutive outputs -------------------------------------------
  int xo[RATE_PER_THREAD], ko[RATE_PER_THREAD];
  bool live[RATE_PER_THREAD];
#pragma unroll
  for (int i = 0; i < RATE_PER_THREAD; ++i) {
    const int place = t + RATE_THREADS * i, n = n_lo + place;
    live[i] = place < to && n >= 0 && n < n_out;
    const int ql = live[i] ? place / nw : 0;
    xo[i] = ql * orig;
    ko[i] = live[i] ? (place - ql * nw) * taps : 0;
  }
  float acc[RATE_PER_THREAD] = {0.f, 0.f, 0.f, 0.f};
  if (TABLE == 2) {
    for (int j = 0; j < taps; ++j) {
      const float k = tab[j];
#pragma unroll
      for (int i = 0; i < RATE_PER_THREAD; ++i) acc[i] = fmaf(k, win[xo[i] + j], acc[i]);
    }
  } else {
    const float* kt = TABLE ? tab : a.kernels;
    for (int j = 0; j < taps; ++j) {
#pragma unroll
      for (int i = 0; i < RATE_PER_THREAD; ++i) acc[i] = fmaf(kt[ko[i] + j], win[xo[i] + j], acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < RATE_PER_THREAD; ++i) {
    const int place = t + RATE_THREADS * i, n = n_lo + place;
    if (live[i])
      o[n] = acc[i];
    else if (place < to && n >= n_out && n < a.fill_to)
      o[n] = 0.f;
  }
}

template <int TABLE>
__device__ __forceinline__ void rate_tile(const RateArgs& a, const float* xr, float* o, int len, int n_out, int tile, float* win_raw, float* tab) {
  rate_tile_staged<TABLE>(a, RateStageF32{xr}, o, len, n_out, tile, win_raw, tab);
}

// values of q per tile: as many as RATE_TILE_OUT outputs and the window budget allow; 0 when not even one fits
inline int rate_tq(int orig, int nw, int taps) {
  const long long by_out = RATE_TILE_OUT / nw, by_win = ((long long)RATE_WINDOW_FLOATS - (taps - 1)) / orig;
  const long long tq = by_out < by_win ? by_out : by_win;
  return tq < 1 ? 0 : (int)tq;
}

inline int check_ratio(const char* what, int orig, int nw, int width, int* taps, int* tq) {
  EBEN_REQUIRE(orig > 0 && nw > 0 && width >= 0, "%s: ratio %d : %d, width %d", what, orig, nw, width);
  const long long tp = 2LL * width + orig;
  EBEN_REQUIRE(tp <= RATE_WINDOW_FLOATS && nw <= RATE_TILE_OUT && rate_tq(orig, nw, (int)tp) >= 1,
               "%s: the ratio %d : %d with %lld taps fits no tile (window of %d floats, %d outputs)", what, orig, nw, tp, RATE_WINDOW_FLOATS, RATE_TILE_OUT);
  *taps = (int)tp;
  *tq = rate_tq(orig, nw, (int)tp);
  return EBEN_OK;
}

// which rate_tile<TABLE> a ratio runs: the table in LDS when it fits, one value per tap when nw == 1 too
inline int rate_table_route(int nw, int taps) { return (long long)nw * taps > RATE_TABLE_FLOATS ? 0 : nw == 1 ? 2 : 1; }

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace
}  // namespace eben
