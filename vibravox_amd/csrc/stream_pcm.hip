// Live sessions in and out as PCM at the caller's rate: the per-slot back end and the PCM front of streaming.StreamPool, one launch each.
//
//   stream_pcm_out_kernel   per piece (one session of one run) what rate_splice_slots_kernel, rate_slots_kernel and pcm_encode_kernel do
//                           one after the other: the tape [carry | new] goes to the slot's twin tape, the outputs of that tape are formed
//                           from an LDS window staged straight from the two sources (the other tape's carry, the run's emitted row), and
//                           each output leaves as PCM16 / PCM24 / PCM32 / FLOAT32 bytes.  The arithmetic is rate_tile.h's, restated because
//                           its store is part of rate_tile_staged: the same phase grid, acc = 0 and acc = fmaf(k[j], x[j], acc) in
//                           ascending j over all taps, zeros by INDEX outside [0, len) -- so the outputs are bit for bit those of
//                           eben_resample_slots.  The conversion is pcm_encode.hip's enc_int, restated.
//   pcm_chunks_in_kernel    corpus.hip's four conversions on mono chunks that lie anywhere in memory (a frame inside a network buffer has
//                           no alignment), read byte by byte.
//
// A tick of 64 sessions writes about 100 KB and reads as much: what these kernels are paid for is being ONE launch each, not vector
// width.  So the window is staged float by float (its two sources have different alignments), the chunks are read byte by byte and
// the stores go out sample by sample (2, 3 or 4 bytes); there is no LDS transpose behind the outputs.
//
// A block of a piece reads only tapes[1 - tape] and src, and writes only tapes[tape] and the image: no launch reads what it writes.
// Grid (tiles of the largest piece, pieces): every block of a piece's column copies a stride of the tape first, then the blocks past the
// piece's own tiles return (before any barrier).
#include <algorithm>

#include "rate_tile.h"

namespace eben {
namespace {

constexpr int SP_KERNARG_BYTES = 3584;   // eben_resample_slots' piece table: the budget of everything passed by value here
constexpr int SP_PASS_TILE = RATE_TILE_OUT;   // outputs per block of a piece that is not resampled

struct SpRatio {
  const float* kernels;
  int orig, nw, taps, tq;
};
struct SpTable {
  EbenStreamPcmPiece p[EBEN_STREAM_PCM_MAX_PIECES];
  SpRatio r[EBEN_RATE_MAX_RATIOS];
};
struct ChunkTable { EbenPcmChunk c[EBEN_PCM_MAX_CHUNKS]; };
static_assert(sizeof(EbenStreamPcmPiece) == 36, "EbenStreamPcmPiece is 36 bytes");
static_assert(sizeof(SpTable) + 64 <= SP_KERNARG_BYTES, "the piece table does not fit the kernel arguments");
static_assert(sizeof(ChunkTable) + 64 <= SP_KERNARG_BYTES, "the chunk table does not fit the kernel arguments");

__host__ __device__ inline int sp_bytes(int format) { return format == EBEN_PCM_S16 ? 2 : format == EBEN_PCM_S24 ? 3 : 4; }

// the stored integer of a sample (pcm_encode.hip's enc_int); *clip counts what left the range
template <int BITS>
__device__ __forceinline__ int sp_int(float x, int* clip) {
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

// output n of a piece whose bytes start at o
__device__ __forceinline__ void sp_store(unsigned char* o, int format, int n, float x, int* clip) {
  if (format == EBEN_PCM_S16) {
    *reinterpret_cast<short*>(o + 2 * (long long)n) = (short)sp_int<16>(x, clip);
  } else if (format == EBEN_PCM_S24) {
    const int v = sp_int<24>(x, clip);
    unsigned char* b = o + 3 * (long long)n;
    b[0] = (unsigned char)v;
    b[1] = (unsigned char)(v >> 8);
    b[2] = (unsigned char)(v >> 16);
  } else if (format == EBEN_PCM_S32) {
    *reinterpret_cast<int*>(o + 4 * (long long)n) = sp_int<32>(x, clip);
  } else {
    *reinterpret_cast<unsigned*>(o + 4 * (long long)n) = __float_as_uint(x);
  }
}

// One tile of one piece: rate_tile_staged with the window staged from [in_row[prev_off ...] | src_row] and the store replaced.
// TABLE as in rate_tile.h.  `win`: RATE_WINDOW_FLOATS floats, `tab`: RATE_TABLE_FLOATS.
template <int TABLE>
__device__ __forceinline__ void sp_tile(const EbenStreamPcmPiece& pc, const SpRatio& rt, const float* in_row, const float* src_row, unsigned char* o,
                                        int tile, float* win, float* tab, int* clip) {
  const int t = threadIdx.x;
  const int orig = rt.orig, nw = rt.nw, taps = rt.taps;
  const int to = rt.tq * nw;             // outputs of a tile
  const int n_lo = tile * to - pc.p0;    // output index of the tile's place 0 (below 0 in the first tile when p0 > 0)
  const int len = pc.n_carry + pc.n_new, n_out = pc.n_out;
  // ---- stage the window: tape indices [w0, w0 + wlen), zero outside [0, len) ---------------------------------------------------------
  const int w0 = pc.base0 + tile * rt.tq * orig;
  const int wlen = rt.tq * orig + taps - 1;
  for (int s = t; s < wlen; s += RATE_THREADS) {
    const int i = w0 + s;
    float v = 0.f;
    if (i >= 0 && i < len) v = i < pc.n_carry ? in_row[pc.prev_off + i] : src_row[i - pc.n_carry];
    win[s] = v;
  }
  if (TABLE) {
    const int nt = nw * taps;
    for (int s = t; s < nt; s += RATE_THREADS) tab[s] = rt.kernels[s];
  }
  __syncthreads();
  // ---- four outputs per thread, RATE_THREADS apart: consecutive lanes consecutive outputs --------------------------------------------
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
    const float* kt = TABLE ? tab : rt.kernels;
    for (int j = 0; j < taps; ++j) {
#pragma unroll
      for (int i = 0; i < RATE_PER_THREAD; ++i) acc[i] = fmaf(kt[ko[i] + j], win[xo[i] + j], acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < RATE_PER_THREAD; ++i)
    if (live[i]) sp_store(o, pc.format, n_lo + t + RATE_THREADS * i, acc[i], clip);
}

// blockIdx.y = piece, blockIdx.x = tile of that piece; the table route follows the piece's ratio, so it is uniform over the block
__global__ __launch_bounds__(RATE_THREADS) void stream_pcm_out_kernel(float* tape0, float* tape1, int tape_pitch, const float* src, int src_pitch,
                                                                      unsigned char* image, int* clipped, SpTable t) {
  __shared__ float win[RATE_WINDOW_FLOATS];
  __shared__ float tab[RATE_TABLE_FLOATS];
  __shared__ int block_clip;
  const EbenStreamPcmPiece pc = t.p[blockIdx.y];
  const int tid = threadIdx.x;
  const float* src_row = pc.n_new > 0 ? src + (long long)pc.src_row * src_pitch : nullptr;
  unsigned char* o = image + pc.byte_offset;
  int clip = 0;
  if (tid == 0) block_clip = 0;
  if (pc.ratio < 0) {   // the model's rate: the emitted row itself
    const long long n0 = (long long)blockIdx.x * SP_PASS_TILE;
    if (n0 >= pc.n_out) return;
#pragma unroll
    for (int i = 0; i < RATE_PER_THREAD; ++i) {
      const long long n = n0 + tid + RATE_THREADS * i;
      if (n < pc.n_out) sp_store(o, pc.format, (int)n, src_row[n], &clip);
    }
    __syncthreads();
  } else {
    const SpRatio rt = t.r[pc.ratio];
    const long long row = (long long)pc.slot * tape_pitch;
    const float* in_row = (pc.tape ? tape0 : tape1) + row;
    float* out_row = (pc.tape ? tape1 : tape0) + row;
    const int len = pc.n_carry + pc.n_new;
    // the tape the next push carries from: every block of the column takes a stride of it
    for (long long j = (long long)blockIdx.x * RATE_THREADS + tid; j < len; j += (long long)gridDim.x * RATE_THREADS)
      out_row[j] = j < pc.n_carry ? in_row[pc.prev_off + j] : src_row[j - pc.n_carry];
    if ((long long)blockIdx.x * rt.tq * rt.nw >= (long long)pc.p0 + pc.n_out) return;   // past this piece's own tiles (before any barrier)
    if (rt.nw * rt.taps > RATE_TABLE_FLOATS)
      sp_tile<0>(pc, rt, in_row, src_row, o, blockIdx.x, win, tab, &clip);
    else if (rt.nw == 1)
      sp_tile<2>(pc, rt, in_row, src_row, o, blockIdx.x, win, tab, &clip);
    else
      sp_tile<1>(pc, rt, in_row, src_row, o, blockIdx.x, win, tab, &clip);
  }
  // behind a barrier in either branch: block_clip is zero for every thread
  if (clip) atomicAdd(&block_clip, clip);
  __syncthreads();
  if (tid == 0 && block_clip) atomicAdd(clipped + pc.slot, block_clip);
}

// sample i of a mono chunk at any address: corpus.hip's conversions on bytes put together one by one
__device__ __forceinline__ float chunk_sample(const unsigned char* base, int format, int i) {
  if (format == EBEN_PCM_S16) {
    const unsigned char* b = base + 2 * (long long)i;
    return (float)((int)b[0] | ((int)(signed char)b[1] << 8)) * 0x1p-15f;
  }
  if (format == EBEN_PCM_S24) {
    const unsigned char* b = base + 3 * (long long)i;
    return (float)((int)b[0] | ((int)b[1] << 8) | ((int)(signed char)b[2] << 16)) * 0x1p-23f;
  }
  const unsigned char* b = base + 4 * (long long)i;
  const unsigned u = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
  if (format == EBEN_PCM_S32) return (float)(int)u * 0x1p-31f;
  return __uint_as_float(u);
}

// blockIdx.y = chunk, a block owns EBEN_PCM_CHUNK_TILE consecutive samples of it
__global__ __launch_bounds__(256) void pcm_chunks_in_kernel(float* dst, int pitch, ChunkTable t) {
  const EbenPcmChunk c = t.c[blockIdx.y];
  const long long n0 = (long long)blockIdx.x * EBEN_PCM_CHUNK_TILE;
  if (n0 >= c.n) return;
  const unsigned char* base = static_cast<const unsigned char*>(c.bytes);
  float* o = dst + (long long)c.dst_row * pitch;
#pragma unroll
  for (int k = 0; k < EBEN_PCM_CHUNK_TILE / 256; ++k) {
    const long long n = n0 + threadIdx.x + 256 * k;
    if (n < c.n) o[n] = chunk_sample(base, c.format, (int)n);
  }
}

inline bool sp_aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// byte extents [a, a + na) and [b, b + nb); an empty or null one overlaps nothing
inline bool sp_overlap(const void* a, long long na, const void* b, long long nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (unsigned long long)nb && b0 < a0 + (unsigned long long)na;
}

struct SpSpan {
  long long lo, hi;
  int piece;
};

// eben_resample_slots' check of one piece against its tape (rate.hip's check_piece without an output pitch: the outputs go to the image)
int sp_check_piece(int i, int len, int n_out, int p0, int base0, int end, int orig, int nw, int width, int taps) {
  const char* who = "stream_pcm_out";
  EBEN_REQUIRE(p0 >= 0 && p0 < nw, "%s: piece %d: phase %d of %d", who, i, p0, nw);
  EBEN_REQUIRE(base0 >= -RATE_MAX_SAMPLES && base0 <= RATE_MAX_SAMPLES, "%s: piece %d: base index %d", who, i, base0);
  if (n_out == 0) return EBEN_OK;
  const long long g_last = (long long)p0 + n_out - 1, q_last = g_last / nw, p_last = g_last - q_last * nw;
  const long long base_last = base0 + q_last * orig;
  EBEN_REQUIRE(base_last + taps <= (long long)RATE_MAX_SAMPLES, "%s: piece %d: the last output's taps start at %lld", who, i, base_last);
  if (end)   // the right end is the signal's own: output n exists when n * orig < nw * total, in buffer terms
    EBEN_REQUIRE((base_last + width) * nw + p_last * orig < (long long)nw * len, "%s: piece %d: %d outputs reach past the signal's %d samples", who, i, n_out,
                 len);
  else       // the signal goes on: every tap of every output lies inside the tape
    EBEN_REQUIRE(base_last + taps <= len, "%s: piece %d: %d outputs read up to index %lld of a tape of %d that is not the signal's end", who, i, n_out,
                 base_last + taps - 1, len);
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_stream_pcm_plan(int orig, int nw, int width, int* out, int n) {
  EBEN_REQUIRE(out && n >= 3, "stream_pcm_plan: needs room for 3 values");
  int taps = 0, tq = 0;
  if (int rc = check_ratio("stream_pcm_plan", orig, nw, width, &taps, &tq)) return rc;
  out[0] = tq * nw;
  out[1] = tq * orig + taps - 1;
  out[2] = rate_table_route(nw, taps);
  return EBEN_OK;
}

extern "C" int eben_stream_pcm_out(float* tape0, float* tape1, int tape_pitch, int slots, const float* src, int src_pitch, int src_rows,
                                   const EbenRateRatio* ratios, int n_ratios, void* image, long long image_bytes, int32_t* clipped,
                                   const EbenStreamPcmPiece* pieces, int count, void* stream) {
  const char* what = "stream_pcm_out";
  EBEN_REQUIRE(count >= 0 && count <= EBEN_STREAM_PCM_MAX_PIECES, "%s: %d pieces, at most %d", what, count, EBEN_STREAM_PCM_MAX_PIECES);
  if (count == 0) return EBEN_OK;
  EBEN_REQUIRE(pieces, "%s: null piece table", what);
  EBEN_REQUIRE(image && clipped, "%s: null image or clipped table", what);
  EBEN_REQUIRE(sp_aligned(image, 16) && aligned4(clipped) && aligned4(tape0) && aligned4(tape1) && aligned4(src),
               "%s: misaligned pointer (image to 16 bytes, the others to 4)", what);
  EBEN_REQUIRE(slots > 0 && slots <= EBEN_STREAM_MAX_SLOTS, "%s: %d slots (1 ... %d)", what, slots, EBEN_STREAM_MAX_SLOTS);
  EBEN_REQUIRE(image_bytes >= 0 && image_bytes < 0x80000000LL, "%s: an image of %lld bytes (below 2^31)", what, image_bytes);
  EBEN_REQUIRE(n_ratios >= 0 && n_ratios <= EBEN_RATE_MAX_RATIOS, "%s: %d ratios (0 ... %d)", what, n_ratios, EBEN_RATE_MAX_RATIOS);
  SpTable t;
  bool used[EBEN_RATE_MAX_RATIOS] = {}, seen[EBEN_STREAM_MAX_SLOTS] = {};
  int width_of[EBEN_RATE_MAX_RATIOS] = {};
  bool any_rated = false, any_new = false;
  long long tiles = 0;
  SpSpan spans[EBEN_STREAM_PCM_MAX_PIECES];
  int n_spans = 0;
  for (int i = 0; i < count; ++i) {
    const EbenStreamPcmPiece& p = pieces[i];
    EBEN_REQUIRE(p.slot < slots, "%s: piece %d names slot %d of %d", what, i, p.slot, slots);
    EBEN_REQUIRE(!seen[p.slot], "%s: two pieces on slot %d", what, p.slot);
    seen[p.slot] = true;
    EBEN_REQUIRE(p.format <= EBEN_PCM_F32, "%s: piece %d has the unknown format %d", what, i, p.format);
    EBEN_REQUIRE(p.ratio >= -1 && p.ratio < n_ratios, "%s: piece %d names ratio %d of %d (-1: none)", what, i, p.ratio, n_ratios);
    EBEN_REQUIRE(p.tape <= 1 && p.end <= 1, "%s: piece %d writes tape %d with end %d (0 or 1 each)", what, i, p.tape, p.end);
    EBEN_REQUIRE(p.n_carry >= 0 && p.n_new >= 0 && p.n_out >= 0, "%s: piece %d: carry %d, new %d, %d outputs", what, i, p.n_carry, p.n_new, p.n_out);
    if (p.n_new > 0) {
      EBEN_REQUIRE(src, "%s: null src with %d new samples in piece %d", what, p.n_new, i);
      EBEN_REQUIRE(src_pitch > 0 && src_rows > 0 && p.n_new <= src_pitch, "%s: piece %d: %d new samples past src's pitch %d", what, i, p.n_new, src_pitch);
      EBEN_REQUIRE(p.src_row < src_rows, "%s: piece %d names src row %d of %d", what, i, p.src_row, src_rows);
      any_new = true;
    }
    long long to = SP_PASS_TILE, places = p.n_out;
    if (p.ratio < 0) {
      EBEN_REQUIRE(p.n_carry == 0 && p.n_out == p.n_new, "%s: piece %d is not resampled, yet carries %d samples or has %d outputs of %d new samples", what, i,
                   p.n_carry, p.n_out, p.n_new);
    } else {
      EBEN_REQUIRE(ratios, "%s: null ratio table", what);
      EBEN_REQUIRE(tape0 && tape1, "%s: null tape", what);
      EBEN_REQUIRE(tape_pitch > 0 && tape_pitch <= RATE_MAX_SAMPLES, "%s: a tape pitch of %d", what, tape_pitch);
      const EbenRateRatio& r = ratios[p.ratio];
      if (!used[p.ratio]) {
        EBEN_REQUIRE(r.kernels && aligned4(r.kernels), "%s: a null or misaligned table of ratio %d", what, p.ratio);
        int taps = 0, tq = 0;
        if (int rc = check_ratio(what, r.orig, r.nw, r.width, &taps, &tq)) return rc;
        t.r[p.ratio] = SpRatio{r.kernels, r.orig, r.nw, taps, tq};
        width_of[p.ratio] = r.width;
        used[p.ratio] = true;
      }
      const SpRatio& sr = t.r[p.ratio];
      const long long len = (long long)p.n_carry + p.n_new;
      EBEN_REQUIRE(len > 0 && len <= tape_pitch, "%s: piece %d: carry %d + new %d outside 1 ... the tape's pitch %d", what, i, p.n_carry, p.n_new, tape_pitch);
      if (p.n_carry > 0)
        EBEN_REQUIRE(p.prev_off >= 0 && (long long)p.prev_off + p.n_carry <= tape_pitch, "%s: piece %d: prev offset %d + carry %d past the pitch %d", what, i,
                     p.prev_off, p.n_carry, tape_pitch);
      if (int rc = sp_check_piece(i, (int)len, p.n_out, p.p0, p.base0, p.end, sr.orig, sr.nw, width_of[p.ratio], sr.taps)) return rc;
      to = (long long)sr.tq * sr.nw;
      places = (long long)p.p0 + p.n_out;
      any_rated = true;
    }
    EBEN_REQUIRE(p.byte_offset >= 0 && (p.byte_offset & 15) == 0, "%s: piece %d starts at byte %d, not a multiple of 16", what, i, p.byte_offset);
    const long long bytes = (long long)p.n_out * sp_bytes(p.format);
    EBEN_REQUIRE(p.byte_offset + bytes <= image_bytes, "%s: piece %d writes the bytes [%d, %lld) of an image of %lld", what, i, p.byte_offset,
                 p.byte_offset + bytes, image_bytes);
    if (bytes) spans[n_spans++] = SpSpan{p.byte_offset, p.byte_offset + bytes, i};
    long long mine = (places + to - 1) / to;
    if (p.ratio >= 0 && mine < 1) mine = 1;   // the tape is written whatever the outputs
    tiles = mine > tiles ? mine : tiles;
    t.p[i] = p;
  }
  std::sort(spans, spans + n_spans, [](const SpSpan& a, const SpSpan& b) { return a.lo < b.lo; });
  for (int k = 1; k < n_spans; ++k)
    EBEN_REQUIRE(spans[k].lo >= spans[k - 1].hi, "%s: pieces %d and %d overlap in the image: bytes [%lld, %lld) and [%lld, %lld)", what, spans[k - 1].piece,
                 spans[k].piece, spans[k - 1].lo, spans[k - 1].hi, spans[k].lo, spans[k].hi);
  // extents: the tapes, the image and clipped are written; src and the tables are read
  const long long tape_b = any_rated ? 4LL * slots * tape_pitch : 0, src_b = any_new ? 4LL * src_rows * src_pitch : 0, clip_b = 4LL * slots;
  const void* tp0 = any_rated ? tape0 : nullptr;
  const void* tp1 = any_rated ? tape1 : nullptr;
  EBEN_REQUIRE(!sp_overlap(tp0, tape_b, tp1, tape_b), "%s: the two tapes overlap", what);
  EBEN_REQUIRE(!sp_overlap(tp0, tape_b, src, src_b) && !sp_overlap(tp1, tape_b, src, src_b), "%s: a tape overlaps src", what);
  EBEN_REQUIRE(!sp_overlap(image, image_bytes, tp0, tape_b) && !sp_overlap(image, image_bytes, tp1, tape_b) && !sp_overlap(image, image_bytes, src, src_b),
               "%s: the image overlaps a tape or src", what);
  EBEN_REQUIRE(!sp_overlap(clipped, clip_b, image, image_bytes) && !sp_overlap(clipped, clip_b, tp0, tape_b) && !sp_overlap(clipped, clip_b, tp1, tape_b) &&
                   !sp_overlap(clipped, clip_b, src, src_b),
               "%s: the clipped table overlaps the image, a tape or src", what);
  for (int k = 0; k < EBEN_RATE_MAX_RATIOS; ++k) {
    if (!used[k]) continue;
    const long long tab_b = 4LL * t.r[k].nw * t.r[k].taps;
    EBEN_REQUIRE(!sp_overlap(t.r[k].kernels, tab_b, tp0, tape_b) && !sp_overlap(t.r[k].kernels, tab_b, tp1, tape_b) &&
                     !sp_overlap(t.r[k].kernels, tab_b, image, image_bytes) && !sp_overlap(t.r[k].kernels, tab_b, clipped, clip_b),
                 "%s: the table of ratio %d overlaps a tape, the image or the clipped table", what, k);
  }
  if (tiles == 0) return EBEN_OK;   // nothing resampled and no output anywhere
  for (int k = 0; k < EBEN_RATE_MAX_RATIOS; ++k)
    if (!used[k]) t.r[k] = SpRatio{nullptr, 1, 1, 1, 1};
  for (int i = count; i < EBEN_STREAM_PCM_MAX_PIECES; ++i) t.p[i] = EbenStreamPcmPiece{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0};
  EBEN_REQUIRE(tiles <= 0x7fffffffLL, "%s: grid of %lld tiles", what, tiles);
  hipLaunchKernelGGL(stream_pcm_out_kernel, dim3((unsigned)tiles, (unsigned)count), dim3(RATE_THREADS), 0, as_stream(stream), tape0, tape1, tape_pitch, src,
                     src_pitch, static_cast<unsigned char*>(image), clipped, t);
  EBEN_CHECK_LAUNCH("stream_pcm_out_kernel");
  return EBEN_OK;
}

extern "C" int eben_pcm_chunks_in(const EbenPcmChunk* chunks, int count, float* dst, int rows, int pitch, void* stream) {
  const char* what = "pcm_chunks_in";
  EBEN_REQUIRE(count >= 0 && count <= EBEN_PCM_MAX_CHUNKS, "%s: %d chunks, at most %d", what, count, EBEN_PCM_MAX_CHUNKS);
  if (count == 0) return EBEN_OK;
  EBEN_REQUIRE(chunks, "%s: null chunk table", what);
  EBEN_REQUIRE(dst && aligned4(dst), "%s: a null or misaligned dst", what);
  EBEN_REQUIRE(rows > 0 && pitch > 0 && pitch <= RATE_MAX_SAMPLES, "%s: dst of %d rows at pitch %d", what, rows, pitch);
  ChunkTable t;
  int longest = 0;
  const long long dst_b = 4LL * rows * pitch;
  for (int i = 0; i < count; ++i) {
    const EbenPcmChunk& c = chunks[i];
    EBEN_REQUIRE(c.format >= EBEN_PCM_S16 && c.format <= EBEN_PCM_F32, "%s: chunk %d has the unknown format %d", what, i, c.format);
    EBEN_REQUIRE(c.n >= 0 && c.n <= pitch, "%s: chunk %d has %d samples (0 ... the pitch %d)", what, i, c.n, pitch);
    EBEN_REQUIRE(c.bytes || c.n == 0, "%s: chunk %d: null bytes with %d samples", what, i, c.n);
    EBEN_REQUIRE(c.dst_row >= 0 && c.dst_row < rows, "%s: chunk %d names row %d of %d", what, i, c.dst_row, rows);
    for (int j = 0; j < i; ++j) EBEN_REQUIRE(chunks[j].dst_row != c.dst_row, "%s: chunks %d and %d both write row %d", what, j, i, c.dst_row);
    EBEN_REQUIRE(!sp_overlap(c.bytes, (long long)c.n * sp_bytes(c.format), dst, dst_b), "%s: the bytes of chunk %d overlap dst", what, i);
    longest = c.n > longest ? c.n : longest;
    t.c[i] = c;
  }
  if (longest == 0) return EBEN_OK;
  for (int i = count; i < EBEN_PCM_MAX_CHUNKS; ++i) t.c[i] = EbenPcmChunk{nullptr, 0, 0, 0};
  hipLaunchKernelGGL(pcm_chunks_in_kernel, dim3((unsigned)((longest + EBEN_PCM_CHUNK_TILE - 1) / EBEN_PCM_CHUNK_TILE), (unsigned)count), dim3(256), 0,
                     as_stream(stream), dst, pitch, t);
  EBEN_CHECK_LAUNCH("pcm_chunks_in_kernel");
  return EBEN_OK;
}
