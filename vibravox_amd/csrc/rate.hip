// Input at the recording's rate: windowed-sinc resampling of ragged rows and of a stream's tape, on one kernel family.
//
// The arithmetic is eben_resample's (direct.hip), unchanged: with the rates reduced to orig : nw and taps = 2 * width + orig,
//
//   y[q * nw + p] = sum_{j < taps} kernels[p][j] * x[q * orig + j - width]        fp32, fmaf, ascending j, indices outside the signal skipped
//
// so a row's result is bit for bit what eben_resample gives on that row alone.  (A skipped index and a staged zero are the same thing:
// the accumulator starts at +0 and is never -0, so fmaf(k, 0, acc) == acc for every finite k.  The staging substitutes the zero by INDEX,
// never by value: what lies outside a row may be NaN.)
//
// Buffer view.  A row's buffer holds the samples [pos0, pos0 + len) of a signal that starts at stream position 0; pos0 itself stays on
// the host.  The launch gets the phase p0 of its first output and the buffer index base0 of that output's tap 0
// (q0 * orig - width - pos0); output n of the launch is g = p0 + n in the launch's own phase grid, q = g / nw, p = g % nw, its tap j at
// buffer index base0 + q * orig + j.  Indices below 0 or at / behind len are zero; every index is a buffer-relative 32-bit value.  len
// is clamped into [0, l_in_buf] whatever the table holds: nothing outside [0, l_in_buf) of a row is ever read.
//
// Kernel shape.  A block owns RATE_TQ(orig, nw, taps) values of q of one row = TQ * nw outputs (at most RATE_TILE_OUT, four per thread),
// stages their TQ * orig + taps - 1 input samples into LDS once -- 16-byte loads over the part of the window that is aligned in memory
// and lies inside the row, the LDS copy shifted so that those land on 16-byte LDS slots -- and the table beside them when nw * taps fits
// RATE_TABLE_FLOATS (48 k -> 16 k: 41 floats; 44.1 k -> 16 k: 160 x 475 floats do not fit and are read through L2).  With nw == 1 the four
// outputs of a thread share each table value.  eben_resample_plan tells the tile constants without launching anything.
//
// Per-slot forms (streaming.StreamPool with input_rates): independent sessions in the slots of one state, each at its own phase, ratio
// and parity.  eben_rate_splice_slots and eben_resample_slots take a table of per-slot descriptors from host memory, validate every
// one, and hand the table to the kernel by value; blockIdx.y is the descriptor.  The resampling kernel runs the tile above (rate_tile,
// the same device function) with the piece's own numbers; a block past its piece's tile count returns, and the table route follows
// the piece's ratio, so it is uniform over the block.  The tile itself lives in rate_tile.h: corpus.hip runs it on PCM rows.
#include "rate_tile.h"

namespace eben {
namespace {

template <int TABLE>
__global__ __launch_bounds__(RATE_THREADS) void rate_kernel(RateArgs a) {
  __shared__ __attribute__((aligned(16))) float win_raw[RATE_WINDOW_FLOATS + 4];
  __shared__ float tab[TABLE ? RATE_TABLE_FLOATS : 1];
  const int r = blockIdx.y;
  int len = a.len, n_out = a.n_out;
  if (a.lens) {
    len = a.lens[r];
    len = len < 0 ? 0 : len > a.in_pitch ? a.in_pitch : len;
    n_out = (int)(((long long)a.nw * len + a.orig - 1) / a.orig);   // <= out_pitch: the entry checked the pitch against in_pitch
    if (blockIdx.x == 0 && threadIdx.x == 0) a.out_lens[r] = n_out;
  }
  rate_tile<TABLE>(a, a.x + (long long)r * a.in_pitch, a.out + (long long)r * a.out_pitch + a.first_out, len, n_out, blockIdx.x, win_raw, tab);
}

int launch_rate(const RateArgs& a, int rows, long long places, void* stream, const char* what) {
  const long long tiles = (places + (long long)a.tq * a.nw - 1) / ((long long)a.tq * a.nw);
  EBEN_REQUIRE(tiles >= 1 && tiles <= 0x7fffffffLL, "%s: grid of %lld tiles", what, tiles);
  const dim3 grid((unsigned)tiles, (unsigned)rows), block(RATE_THREADS);
  switch (rate_table_route(a.nw, a.taps)) {
    case 0: hipLaunchKernelGGL(rate_kernel<0>, grid, block, 0, as_stream(stream), a); break;
    case 2: hipLaunchKernelGGL(rate_kernel<2>, grid, block, 0, as_stream(stream), a); break;
    default: hipLaunchKernelGGL(rate_kernel<1>, grid, block, 0, as_stream(stream), a); break;
  }
  EBEN_CHECK_LAUNCH("rate_kernel");
  return EBEN_OK;
}

// ---- per-slot forms: independent sessions in the slots of one state, every slot with its own numbers --------------------------------
// The descriptors travel by value in the kernel arguments, which the runtime limits to RATE_KERNARG_BYTES in all.
constexpr int RATE_KERNARG_BYTES = 4096;
constexpr int RATE_KERNARG_OTHER = 64;   // the pointers and pitches beside a table

struct SpliceTable { EbenRateSplice s[EBEN_RATE_MAX_SPLICES]; };
struct SlotRatio {
  const float* kernels;
  int orig, nw, taps, tq;
};
struct PieceTable {
  EbenRatePiece p[EBEN_RATE_MAX_PIECES];
  SlotRatio r[EBEN_RATE_MAX_RATIOS];
};
static_assert(sizeof(SpliceTable) + RATE_KERNARG_OTHER <= RATE_KERNARG_BYTES, "the splice table does not fit the kernel arguments");
static_assert(sizeof(PieceTable) + RATE_KERNARG_OTHER <= RATE_KERNARG_BYTES, "the piece table does not fit the kernel arguments");

// blockIdx.y = descriptor, thread = one element of its [carry | new]
__global__ __launch_bounds__(256) void rate_splice_slots_kernel(float* __restrict__ tape0, float* __restrict__ tape1, int tape_pitch,
                                                                const float* __restrict__ src, int src_pitch, SpliceTable t) {
  const EbenRateSplice d = t.s[blockIdx.y];
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= d.n_carry + d.n_new) return;
  const long long row = (long long)d.slot * tape_pitch;
  const float* in = d.tape ? tape0 : tape1;
  float* out = d.tape ? tape1 : tape0;
  out[row + j] = j < d.n_carry ? in[row + d.prev_off + j] : src[(long long)d.src_row * src_pitch + (j - d.n_carry)];
}

// blockIdx.y = piece, blockIdx.x = tile of that piece; the table route follows the piece's ratio, so it is uniform over the block
__global__ __launch_bounds__(RATE_THREADS) void rate_slots_kernel(const float* tape0, const float* tape1, int tape_pitch, float* fifo0, float* fifo1,
                                                                  int fifo_pitch, PieceTable t) {
  __shared__ __attribute__((aligned(16))) float win_raw[RATE_WINDOW_FLOATS + 4];
  __shared__ float tab[RATE_TABLE_FLOATS];
  const EbenRatePiece pc = t.p[blockIdx.y];
  const SlotRatio rt = t.r[pc.ratio];
  if ((long long)blockIdx.x * rt.tq * rt.nw >= (long long)pc.p0 + pc.n_out) return;   // past this piece's own tiles (before any barrier)
  const RateArgs a{nullptr, rt.kernels, nullptr, nullptr, nullptr, pc.len, tape_pitch, fifo_pitch, rt.orig, rt.nw, rt.taps, rt.tq, pc.p0, pc.base0,
                   pc.first_out, pc.n_out, 0};
  const float* xr = (pc.tape ? tape1 : tape0) + (long long)pc.slot * tape_pitch;
  float* o = (pc.fifo ? fifo1 : fifo0) + (long long)pc.slot * fifo_pitch + pc.first_out;
  if (rt.nw * rt.taps > RATE_TABLE_FLOATS)
    rate_tile<0>(a, xr, o, pc.len, pc.n_out, blockIdx.x, win_raw, tab);
  else if (rt.nw == 1)
    rate_tile<2>(a, xr, o, pc.len, pc.n_out, blockIdx.x, win_raw, tab);
  else
    rate_tile<1>(a, xr, o, pc.len, pc.n_out, blockIdx.x, win_raw, tab);
}

inline bool overlaps(const float* a, long long na, const float* b, long long nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + 4ull * (unsigned long long)nb && b0 < a0 + 4ull * (unsigned long long)na;
}

// One piece's numbers against its tape and its output row: eben_resample_stream's checks of its launch and eben_resample_slots' of every
// piece.  `who` leads the message ("resample_stream", "resample_slots: piece 3").
int check_piece(const char* who, int len, int tape_pitch, int out_pitch, int first_out, int n_out, int p0, int base0, int end, int orig, int nw, int width,
                int taps) {
  EBEN_REQUIRE(len >= 0 && len <= tape_pitch, "%s: a tape of %d samples at pitch %d", who, len, tape_pitch);
  EBEN_REQUIRE(first_out >= 0 && n_out >= 0 && (long long)first_out + n_out <= out_pitch, "%s: outputs [%d, %d + %d) past the pitch %d", who, first_out,
               first_out, n_out, out_pitch);
  EBEN_REQUIRE(p0 >= 0 && p0 < nw, "%s: phase %d of %d", who, p0, nw);
  EBEN_REQUIRE(base0 >= -RATE_MAX_SAMPLES && base0 <= RATE_MAX_SAMPLES, "%s: base index %d", who, base0);
  if (n_out == 0) return EBEN_OK;
  const long long g_last = (long long)p0 + n_out - 1, q_last = g_last / nw, p_last = g_last - q_last * nw;
  const long long base_last = base0 + q_last * orig;
  EBEN_REQUIRE(base_last + taps <= (long long)RATE_MAX_SAMPLES, "%s: the last output's taps start at %lld", who, base_last);
  if (end)   // the right end is the signal's own: output n exists when n * orig < nw * total, in buffer terms
    EBEN_REQUIRE((base_last + width) * nw + p_last * orig < (long long)nw * len, "%s: %d outputs reach past the signal's %d samples", who, n_out, len);
  else       // the signal goes on: every tap of every output lies inside the tape
    EBEN_REQUIRE(base_last + taps <= len, "%s: %d outputs read up to index %lld of a tape of %d that is not the signal's end", who, n_out,
                 base_last + taps - 1, len);
  return EBEN_OK;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_resample_plan(int orig, int nw, int width, int* out, int n) {
  EBEN_REQUIRE(out && n >= 4, "resample_plan: needs room for 4 values");
  int taps = 0, tq = 0;
  if (int rc = check_ratio("resample_plan", orig, nw, width, &taps, &tq)) return rc;
  out[0] = tq;
  out[1] = tq * nw;
  out[2] = tq * orig + taps - 1;
  out[3] = (long long)nw * taps <= RATE_TABLE_FLOATS ? 1 : 0;
  return EBEN_OK;
}

extern "C" int eben_resample_ragged(const float* x, const int32_t* lens, const float* kernels, float* out, int32_t* out_lens, int rows,
                                    int l_in_buf, int l_out_buf, int orig, int nw, int width, void* stream) {
  EBEN_REQUIRE(x && lens && kernels && out && out_lens, "resample_ragged: null pointer");
  EBEN_REQUIRE(aligned4(x) && aligned4(lens) && aligned4(kernels) && aligned4(out) && aligned4(out_lens), "resample_ragged: misaligned pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535, "resample_ragged: %d rows (1 ... 65535)", rows);
  int taps = 0, tq = 0;
  if (int rc = check_ratio("resample_ragged", orig, nw, width, &taps, &tq)) return rc;
  EBEN_REQUIRE(l_in_buf > 0 && l_in_buf <= RATE_MAX_SAMPLES && l_out_buf > 0 && l_out_buf <= RATE_MAX_SAMPLES,
               "resample_ragged: rows of %d samples in, %d out (1 ... %d)", l_in_buf, l_out_buf, RATE_MAX_SAMPLES);
  const long long need = ((long long)nw * l_in_buf + orig - 1) / orig;
  EBEN_REQUIRE(l_out_buf >= need, "resample_ragged: l_out_buf %d below ceil(%d * %d / %d) = %lld", l_out_buf, nw, l_in_buf, orig, need);
  RateArgs a{x, kernels, out, lens, out_lens, 0, l_in_buf, l_out_buf, orig, nw, taps, tq, 0, -width, 0, 0, l_out_buf};
  return launch_rate(a, rows, l_out_buf, stream, "resample_ragged");
}

extern "C" int eben_resample_stream(const float* tape, const float* kernels, float* out, int rows, int tape_pitch, int len, int out_pitch,
                                    int first_out, int n_out, int p0, int base0, int end, int orig, int nw, int width, void* stream) {
  EBEN_REQUIRE(tape && kernels && out, "resample_stream: null pointer");
  EBEN_REQUIRE(aligned4(tape) && aligned4(kernels) && aligned4(out), "resample_stream: misaligned pointer");
  EBEN_REQUIRE(rows > 0 && rows <= 65535, "resample_stream: %d rows (1 ... 65535)", rows);
  int taps = 0, tq = 0;
  if (int rc = check_ratio("resample_stream", orig, nw, width, &taps, &tq)) return rc;
  EBEN_REQUIRE(tape_pitch > 0 && tape_pitch <= RATE_MAX_SAMPLES, "resample_stream: a tape of %d samples at pitch %d", len, tape_pitch);
  EBEN_REQUIRE(out_pitch > 0 && out_pitch <= RATE_MAX_SAMPLES, "resample_stream: outputs [%d, %d + %d) past the pitch %d", first_out, first_out, n_out,
               out_pitch);
  if (int rc = check_piece("resample_stream", len, tape_pitch, out_pitch, first_out, n_out, p0, base0, end, orig, nw, width, taps)) return rc;
  if (n_out == 0) return EBEN_OK;
  RateArgs a{tape, kernels, out, nullptr, nullptr, len, tape_pitch, out_pitch, orig, nw, taps, tq, p0, base0, first_out, n_out, 0};
  return launch_rate(a, rows, (long long)p0 + n_out, stream, "resample_stream");
}

extern "C" int eben_rate_splice_slots(float* tape0, float* tape1, int tape_pitch, int slots, const float* src, int src_pitch, int src_rows,
                                      const EbenRateSplice* splices, int count, void* stream) {
  EBEN_REQUIRE(count >= 0 && count <= EBEN_RATE_MAX_SPLICES, "rate_splice_slots: %d splices, at most %d", count, EBEN_RATE_MAX_SPLICES);
  if (count == 0) return EBEN_OK;
  EBEN_REQUIRE(splices, "rate_splice_slots: null splice table");
  EBEN_REQUIRE(tape0 && tape1, "rate_splice_slots: null tape");
  EBEN_REQUIRE(aligned4(tape0) && aligned4(tape1) && aligned4(src), "rate_splice_slots: misaligned pointer");
  EBEN_REQUIRE(slots > 0 && slots <= EBEN_STREAM_MAX_SLOTS, "rate_splice_slots: %d slots (1 ... %d)", slots, EBEN_STREAM_MAX_SLOTS);
  EBEN_REQUIRE(tape_pitch > 0 && tape_pitch <= RATE_MAX_SAMPLES, "rate_splice_slots: a tape pitch of %d", tape_pitch);
  SpliceTable t;
  bool seen[EBEN_STREAM_MAX_SLOTS] = {};
  int longest = 0, any_new = 0;
  for (int i = 0; i < count; ++i) {
    const EbenRateSplice& d = splices[i];
    EBEN_REQUIRE(d.slot >= 0 && d.slot < slots, "rate_splice_slots: splice %d names slot %d of %d", i, d.slot, slots);
    EBEN_REQUIRE(!seen[d.slot], "rate_splice_slots: two splices on slot %d", d.slot);
    seen[d.slot] = true;
    EBEN_REQUIRE(d.tape == 0 || d.tape == 1, "rate_splice_slots: splice %d writes tape %d (0 or 1)", i, d.tape);
    EBEN_REQUIRE(d.n_carry >= 0 && d.n_new >= 0 && (long long)d.n_carry + d.n_new > 0, "rate_splice_slots: splice %d: carry %d, new %d", i, d.n_carry,
                 d.n_new);
    EBEN_REQUIRE((long long)d.n_carry + d.n_new <= tape_pitch, "rate_splice_slots: splice %d: carry %d + new %d past the tape's pitch %d", i, d.n_carry,
                 d.n_new, tape_pitch);
    if (d.n_carry > 0)
      EBEN_REQUIRE(d.prev_off >= 0 && (long long)d.prev_off + d.n_carry <= tape_pitch, "rate_splice_slots: splice %d: prev offset %d + carry %d past the pitch %d",
                   i, d.prev_off, d.n_carry, tape_pitch);
    if (d.n_new > 0) {
      EBEN_REQUIRE(src, "rate_splice_slots: null src with %d new samples in splice %d", d.n_new, i);
      EBEN_REQUIRE(src_pitch > 0 && src_rows > 0 && d.n_new <= src_pitch, "rate_splice_slots: splice %d: %d new samples past src's pitch %d", i, d.n_new,
                   src_pitch);
      EBEN_REQUIRE(d.src_row >= 0 && d.src_row < src_rows, "rate_splice_slots: splice %d names src row %d of %d", i, d.src_row, src_rows);
      any_new = 1;
    }
    t.s[i] = d;
    longest = d.n_carry + d.n_new > longest ? d.n_carry + d.n_new : longest;
  }
  const long long tape_n = (long long)slots * tape_pitch;
  EBEN_REQUIRE(!overlaps(tape0, tape_n, tape1, tape_n), "rate_splice_slots: the two tapes overlap");
  if (any_new) {
    const long long src_n = (long long)src_rows * src_pitch;
    EBEN_REQUIRE(!overlaps(tape0, tape_n, src, src_n) && !overlaps(tape1, tape_n, src, src_n), "rate_splice_slots: a tape overlaps src");
  }
  for (int i = count; i < EBEN_RATE_MAX_SPLICES; ++i) t.s[i] = EbenRateSplice{0, 0, 0, 0, 0, 0};
  hipLaunchKernelGGL(rate_splice_slots_kernel, dim3((unsigned)((longest + 255) / 256), (unsigned)count), dim3(256), 0, as_stream(stream), tape0, tape1,
                     tape_pitch, src, src_pitch, t);
  EBEN_CHECK_LAUNCH("rate_splice_slots_kernel");
  return EBEN_OK;
}

extern "C" int eben_resample_slots(const float* tape0, const float* tape1, int tape_pitch, float* fifo0, float* fifo1, int fifo_pitch, int slots,
                                   const EbenRateRatio* ratios, int n_ratios, const EbenRatePiece* pieces, int count, void* stream) {
  EBEN_REQUIRE(count >= 0 && count <= EBEN_RATE_MAX_PIECES, "resample_slots: %d pieces, at most %d", count, EBEN_RATE_MAX_PIECES);
  if (count == 0) return EBEN_OK;
  EBEN_REQUIRE(pieces && ratios, "resample_slots: null piece or ratio table");
  EBEN_REQUIRE(tape0 && tape1 && fifo0 && fifo1, "resample_slots: null tape or FIFO buffer");
  EBEN_REQUIRE(aligned4(tape0) && aligned4(tape1) && aligned4(fifo0) && aligned4(fifo1), "resample_slots: misaligned pointer");
  EBEN_REQUIRE(slots > 0 && slots <= EBEN_STREAM_MAX_SLOTS, "resample_slots: %d slots (1 ... %d)", slots, EBEN_STREAM_MAX_SLOTS);
  EBEN_REQUIRE(n_ratios > 0 && n_ratios <= EBEN_RATE_MAX_RATIOS, "resample_slots: %d ratios (1 ... %d)", n_ratios, EBEN_RATE_MAX_RATIOS);
  EBEN_REQUIRE(tape_pitch > 0 && tape_pitch <= RATE_MAX_SAMPLES && fifo_pitch > 0 && fifo_pitch <= RATE_MAX_SAMPLES,
               "resample_slots: a tape pitch of %d, a FIFO pitch of %d", tape_pitch, fifo_pitch);
  PieceTable t;
  bool used[EBEN_RATE_MAX_RATIOS] = {};
  int kept = 0;
  long long tiles = 0;
  for (int i = 0; i < count; ++i) {
    const EbenRatePiece& p = pieces[i];
    EBEN_REQUIRE(p.slot < slots, "resample_slots: piece %d names slot %d of %d", i, p.slot, slots);
    EBEN_REQUIRE(p.ratio < n_ratios, "resample_slots: piece %d names ratio %d of %d", i, p.ratio, n_ratios);
    EBEN_REQUIRE(p.tape <= 1 && p.fifo <= 1, "resample_slots: piece %d reads tape %d, writes FIFO buffer %d (0 or 1)", i,
                 p.tape, p.fifo);
    const EbenRateRatio& r = ratios[p.ratio];
    if (!used[p.ratio]) {
      EBEN_REQUIRE(r.kernels && aligned4(r.kernels), "resample_slots: a null or misaligned table of ratio %d", p.ratio);
      int taps = 0, tq = 0;
      if (int rc = check_ratio("resample_slots", r.orig, r.nw, r.width, &taps, &tq)) return rc;
      t.r[p.ratio] = SlotRatio{r.kernels, r.orig, r.nw, taps, tq};
      used[p.ratio] = true;
    }
    const SlotRatio& sr = t.r[p.ratio];
    char who[40];
    snprintf(who, sizeof who, "resample_slots: piece %d", i);
    if (int rc = check_piece(who, p.len, tape_pitch, fifo_pitch, p.first_out, p.n_out, p.p0, p.base0, p.end, sr.orig, sr.nw, r.width, sr.taps)) return rc;
    if (p.n_out == 0) continue;
    for (int j = 0; j < kept; ++j) {
      const EbenRatePiece& o = t.p[j];
      EBEN_REQUIRE(o.slot != p.slot || o.fifo != p.fifo || o.first_out + o.n_out <= p.first_out || p.first_out + p.n_out <= o.first_out,
                   "resample_slots: piece %d writes [%d, %d) of FIFO buffer %d, slot %d, which another piece writes too", i, p.first_out,
                   p.first_out + p.n_out, p.fifo, p.slot);
    }
    t.p[kept++] = p;
    const long long to = (long long)sr.tq * sr.nw, mine = ((long long)p.p0 + p.n_out + to - 1) / to;
    tiles = mine > tiles ? mine : tiles;
  }
  const long long tape_n = (long long)slots * tape_pitch, fifo_n = (long long)slots * fifo_pitch;
  EBEN_REQUIRE(!overlaps(fifo0, fifo_n, fifo1, fifo_n), "resample_slots: the two FIFO buffers overlap");
  const float* outs[2] = {fifo0, fifo1};
  for (const float* f : outs) {
    EBEN_REQUIRE(!overlaps(f, fifo_n, tape0, tape_n) && !overlaps(f, fifo_n, tape1, tape_n), "resample_slots: a FIFO buffer overlaps a tape");
    for (int k = 0; k < n_ratios; ++k)
      if (used[k])
        EBEN_REQUIRE(!overlaps(f, fifo_n, t.r[k].kernels, (long long)t.r[k].nw * t.r[k].taps), "resample_slots: a FIFO buffer overlaps the table of ratio %d", k);
  }
  if (kept == 0) return EBEN_OK;
  for (int k = 0; k < EBEN_RATE_MAX_RATIOS; ++k)
    if (k >= n_ratios || !used[k]) t.r[k] = SlotRatio{nullptr, 1, 1, 1, 1};
  for (int i = kept; i < EBEN_RATE_MAX_PIECES; ++i) t.p[i] = EbenRatePiece{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  EBEN_REQUIRE(tiles >= 1 && tiles <= 0x7fffffffLL, "resample_slots: grid of %lld tiles", tiles);
  hipLaunchKernelGGL(rate_slots_kernel, dim3((unsigned)tiles, (unsigned)kept), dim3(RATE_THREADS), 0, as_stream(stream), tape0, tape1, tape_pitch, fifo0,
                     fifo1, fifo_pitch, t);
  EBEN_CHECK_LAUNCH("rate_slots_kernel");
  return EBEN_OK;
}
