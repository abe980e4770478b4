// thin_bl.hip -- the thin bundle-layout tap convs (PQMF-band L1-L4, MelGAN L1-L2: reductions of a few k-steps per block), one kernel
// instantiation per direction with the launch's stride fixed at compile time.  Launches whose plan needs more than one channel chunk (the
// 96-row tiles of PQMF-band L2 / L4) stay on tap3_kernel.
//
// tap3_kernel<..., BL = true> serves every bundle-layout launch with ONE body: the forward instantiation carries the input gradients'
// mask / feature-matching epilogues and the phases-as-rows addressing, the multi-chunk tile hand-over and the run-time phase geometry,
// ~10 000 static instructions for launches whose blocks live 15-40k cycles, of which the instruction stream itself is the larger part.
// Here the same plan (Tap3Plan: tiles, weight image, k-step table -- the packed image is shared with tap3) runs on kernels that keep only
// what their direction executes:
//   DIR 0  forward:                bias, LeakyReLU, hi / lo split, row-quad stores (strides 2 and 4, register-staged input tile);
//   DIR 1  phases-as-rows dX:      mask + feature-matching epilogue in the bundle-major row order (pr_order 1), S = pr_S (2 or 4);
//   DIR 2  phase-scatter dX:       mask + feature-matching epilogue, output phases interleaved (stride-2 layers at dilation 3).
// The k-steps, their order, the piece-product order and the fp32 epilogue are tap3_kernel's, operation for operation: the outputs are
// bit-identical to the tap3 path (tests/test_gpu_thin_bl.py compares both).  EBEN_THIN_BL=0 sends these launches back to tap3_kernel.
#include "common.h"
#include "tap3.h"

#include <cstdlib>

namespace eben {
namespace thin {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));   // v_cvt_pk_bf16_f32 (RNE)
}
template <int N> __device__ __forceinline__ void wait_vm() {   // s_waitcnt vmcnt(N) lgkmcnt(0)
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit count");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x70);
}
__device__ u32x4 zero_unit = {0u, 0u, 0u, 0u};   // where the lanes of an input-tile LDS-DMA piece that fall into the zero padding read from

enum { FWD = 0, DX_PR = 1, DX_PS = 2 };

// tap3_kernel's weight chunking and ring for bundle-layout launches (checked against the plan on the host)
constexpr int ksc_of(int np) { return np == 1 ? 4 : 2; }
constexpr int RING = 2;

// FM: 32-row accumulator tiles per block; NP: operand pieces (1 bf16, 2 hi + lo: three products); S: the conv stride of a forward, the
// phases-as-rows stride pr_S of DIR 1 (whose launch has stride 1); unused (1) for DIR 2.  One channel chunk per block (ncc = 1).
template <int FM, int NP, int DIR, int S>
__global__ __launch_bounds__(256, NP >= 2 ? 1 : 2) void thin_bl_kernel(const Tap3Args P) {
  constexpr int NT = 256, BN = 128, BM = FM * 32, KSC = ksc_of(NP);
  constexpr int WCHU = KSC * NP * FM * 64;       // 16-byte units per weight chunk
  constexpr int WU = (WCHU + NT - 1) / NT;       // LDS-DMA instructions per thread and chunk
  constexpr int CS = DIR == FWD ? S : 1;         // stride of the launch's gather
  constexpr bool DMA_X = CS == 1;                // the input tile moves by LDS-DMA (stride 1, one channel chunk)
  constexpr bool DX = DIR != FWD;
  static_assert(WCHU % 64 == 0, "weight chunk must split into whole wave pieces");

  extern __shared__ __attribute__((aligned(16))) u32x4 smem_thin[];
  u32x4* Ws = smem_thin;              // RING x WCHU
  u32x4* Xs = smem_thin + RING * WCHU;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);

  unsigned id;
  {
    const unsigned bid = blockIdx.x, xcd = bid & 7u, idx = bid >> 3;
    id = (xcd < P.xr ? xcd * (P.xq + 1) : P.xr * (P.xq + 1) + (xcd - P.xr) * P.xq) + idx;   // xcd_remap with the host's quotient
  }
  int ph = 0, tt, b, mt, g;
  if (P.id_fast) {
    unsigned qd;
    if constexpr (DIR == DX_PS) { qd = P.m_nph ? __umulhi(id, P.m_nph) : id; ph = (int)(id - qd * (unsigned)P.nph); id = qd; }
    qd = P.m_ntt ? __umulhi(id, P.m_ntt) : id; tt = (int)(id - qd * (unsigned)P.ntt); id = qd;
    qd = P.m_B ? __umulhi(id, P.m_B) : id; b = (int)(id - qd * (unsigned)P.B); id = qd;
    qd = P.m_nmt ? __umulhi(id, P.m_nmt) : id; mt = (int)(id - qd * (unsigned)P.nmt); g = (int)qd;
  } else {
    if constexpr (DIR == DX_PS) { ph = id % P.nph; id /= P.nph; }
    tt = id % P.ntt; id /= P.ntt;
    b = id % P.B; id /= P.B;
    mt = id % P.nmt;
    g = id / P.nmt;
  }
  ph = __builtin_amdgcn_readfirstlane(ph); tt = __builtin_amdgcn_readfirstlane(tt); b = __builtin_amdgcn_readfirstlane(b);
  mt = __builtin_amdgcn_readfirstlane(mt); g = __builtin_amdgcn_readfirstlane(g);
  const int t0 = tt * BN, m0 = mt * BM;

  // phase geometry: the host's table (nph <= 8 here)
  const int J = P.pg[ph].J, nt = P.pg[ph].nt, oo = DIR == DX_PS ? P.pg[ph].oo : 0, minoff = P.pg[ph].minoff, span = P.pg[ph].span;
  const unsigned span_magic = P.pg[ph].span_magic;
  if (t0 >= nt) return;
  const int KS = J * P.CP;
  const int nch = (KS + KSC - 1) / KSC;
  const int q0 = t0 * CS + minoff;
  const int xtot = P.CI_B * span;          // bundle-positions per input tile
  const int XBUF = P.CI_B * P.CSTRIDE;
  const int LOU = NP > 1 ? XBUF + 1 : 0;   // unit offset from the hi tile to the lo tile

  const u32x4* wsrc = P.wp + (long long)ph * P.w_phase + ((long long)g * P.nmt + mt) * P.w_tile;
  typedef const __attribute__((address_space(4))) int* ctab_t;
  ctab_t tab = (ctab_t)(P.tab + (long long)ph * P.tab_phase);

  f32x16 acc[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // ---- input tile: unit (bundle cbn of this group, position qq) of the input planes; bundles past the group's last are zeros ----
  const int CgB = P.Cg >> 3;
  const long long xrowB = ((long long)b * P.CBx + (long long)g * CgB) * P.Lx;
  const bool inside = q0 >= 0 && q0 + span <= P.Lx;

  auto issue_w = [&](int ch) {
    const u32x4* src = wsrc + (long long)ch * WCHU;
    u32x4* dst = Ws + (ch % RING) * WCHU;
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      int idx = u * NT + tid;
      if (WCHU % NT != 0 && idx >= WCHU) idx -= NT;   // wave-uniform: every wave issues WU instructions per chunk
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + idx),
                                       (__attribute__((address_space(3))) void*)(dst + (idx & ~63)), 16, 0, 0);
    }
  };

  // ---- what the epilogue needs besides the accumulators, asked for under the tile staging ----
  int eb = b;
  if constexpr (DX) {
    eb = P.em_seg > 0 ? P.em_map[(int)(b >= P.em_seg) + (int)(b >= 2 * P.em_seg) + (int)(b >= 3 * P.em_seg)] * P.em_seg +
                            (b - ((int)(b >= P.em_seg) + (int)(b >= 2 * P.em_seg) + (int)(b >= 3 * P.em_seg)) * P.em_seg) : b;
  }
  float* Bs = reinterpret_cast<float*>(Xs + NP * (XBUF + 1));   // BM bias values of this block's rows (forward)
  float fk1 = 0.f, fk2 = 0.f;
  const bool fmr = DX && P.fm_sums != nullptr && P.res_rows > 0 && b < P.res_rows;
  if constexpr (!DX) {
    if (tid < BM) {
      const int m = m0 + tid;
      Bs[tid] = P.bias ? P.bias[(long long)g * P.Mg + (m < P.Mg ? m : P.Mg - 1)] : 0.f;
    }
  } else if (fmr) {
    typedef const __attribute__((address_space(4))) float* cf_t;
    const float s1 = ((cf_t)P.fm_sums)[0], s2 = ((cf_t)P.fm_sums)[1];
    fk1 = P.fm_gs / s2; fk2 = P.fm_gs * s1 / (s2 * s2);
  }
  if (nch > 0) {
    issue_w(0);
    if constexpr (DMA_X) {
      // a tile row -- one bundle over `span` consecutive positions -- is a run of consecutive units in the plane and in LDS: pieces of
      // 64 units by LDS-DMA, lanes past the row's end masked off, lanes in the zero padding / past the group's last bundle reading zeros
      const int ppr = (span + 63) >> 6;   // pieces per bundle row
      int bb = 0, pr = __builtin_amdgcn_readfirstlane(tid >> 6);
      while (pr >= ppr) { pr -= ppr; ++bb; }
      while (bb < P.CI_B) {
        const int r = pr * 64 + lane;
        const int qq = q0 + r;
        const bool in = qq >= 0 && qq < P.Lx && bb < CgB;
        const long long idx = xrowB + (long long)(bb < CgB ? bb : 0) * P.Lx + (in ? qq : 0);
        u32x4* d = Xs + bb * P.CSTRIDE + pr * 64;   // uniform
        if (r < span) {
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in ? P.xh + idx : &zero_unit),
                                           (__attribute__((address_space(3))) void*)d, 16, 0, 0);
          if constexpr (NP > 1)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in ? P.xl + idx : &zero_unit),
                                             (__attribute__((address_space(3))) void*)(d + LOU), 16, 0, 0);
        }
        pr += NT / 64;
        while (pr >= ppr) { pr -= ppr; ++bb; }
      }
    } else {
      // strided gather: the tile is staged through registers into the stride's phase rows, two rounds of two units per thread in flight
      struct Round { u32x4 w[2][NP]; int sl[2], ok[2]; };
      auto pro_load = [&](int base, Round& R) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int i = base + tid + u * NT;
          const int bb = (int)__umulhi((unsigned)i, span_magic);
          const int r = i - bb * span;
          int qq = q0 + (i < xtot ? r : 0), ok = 1;
          if (!inside) {
            ok = (int)(qq >= 0) & (int)(qq < P.Lx);
            qq = ok ? qq : 0;
          }
          ok &= (int)(i < xtot);
          const int c0 = i < xtot ? bb : 0;
          ok &= (int)(c0 < CgB);
          const long long idx = xrowB + (long long)(c0 < CgB ? c0 : 0) * P.Lx + qq;
          R.w[u][0] = P.xh[idx];
          if constexpr (NP > 1) R.w[u][1] = P.xl[idx];
          R.ok[u] = ok;
          const int d = r / CS, p = r - d * CS;
          R.sl[u] = i < xtot ? bb * P.CSTRIDE + p * P.PLEN + d : -1;
        }
      };
      auto pro_store = [&](Round& R) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
          if (R.sl[u] >= 0) {
#pragma unroll
            for (int q = 0; q < NP; ++q) Xs[R.sl[u] + q * LOU] = R.ok[u] ? R.w[u][q] : u32x4{0u, 0u, 0u, 0u};
          }
      };
      Round ra, rb;
      if (xtot > 0) pro_load(0, ra);
      for (int base = 0; base < xtot; base += 4 * NT) {
        const bool second = base + 2 * NT < xtot;
        if (second) pro_load(base + 2 * NT, rb);
        pro_store(ra);
        if (second) {
          if (base + 4 * NT < xtot) pro_load(base + 4 * NT, ra);
          pro_store(rb);
        }
      }
    }
  }
  __syncthreads();
  // activation mask (hi plane of the saved embedding) of this lane's outputs, asked for before the reduction (phase-scatter, <= 64 rows)
  constexpr bool PREF = DIR == DX_PS && FM <= 2;
  uint2 pah[PREF ? FM : 1][4];
  if constexpr (PREF) {
    if (P.eh != nullptr) {
      const int tq = t0 + wn * 32 + (lane & 31);
      const unsigned loffq = (((unsigned)(tq < nt ? tq : nt - 1) * (unsigned)P.OS + (unsigned)oo) * 2u + (unsigned)(lane >> 5)) * 8u;
      const long long Lrowq = (long long)P.Ly * 16;
      const char* ehq = reinterpret_cast<const char*>(P.eh) + (long long)eb * P.CBy * Lrowq + ((long long)((g * P.Mg + m0) >> 3)) * Lrowq;
      const int quadsq = (P.Mg - m0 + 7) >> 3;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int q = 4 * i + r4;
          pah[i][r4] = *reinterpret_cast<const uint2*>(ehq + (long long)(q < quadsq ? q : 0) * Lrowq + loffq);
        }
    }
  }

  // ---- reduction: tap3_kernel's chunk loop (RING 2: the next chunk's weights stream under this one's MFMAs; the second half of a
  // chunk's k-steps is held back across the barrier and issued under the next chunk's first fragment reads) ----
  const int lanebase = (lane >> 5) * P.CSTRIDE + wn * 32 + (lane & 31);
  int te[KSC];
#pragma unroll
  for (int ks = 0; ks < KSC; ++ks) te[ks] = nch > 0 ? tab[ks] : 0;
  constexpr int H = KSC >= 2 ? KSC / 2 : 1, H2 = KSC - H;
  u32x4 bvA[H][NP], aA[H][NP][FM], bvB[H2 > 0 ? H2 : 1][NP], aB[H2 > 0 ? H2 : 1][NP][FM];
  auto mma = [&](const u32x4 (&bq)[NP], const u32x4 (&aq)[NP][FM]) {
    // piece products, smallest first: (qw, qx) with qw + qx = lvl
#pragma unroll
    for (int lvl = NP - 1; lvl >= 0; --lvl)
#pragma unroll
      for (int qw = 0; qw < NP; ++qw) {
        const int qx = lvl - qw;
        if (qx < 0 || qx >= NP) continue;
#pragma unroll
        for (int i = 0; i < FM; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, aq[qw][i]), __builtin_bit_cast(bf16x8, bq[qx]), acc[i], 0, 0, 0);
      }
  };
  for (int ch = 0; ch < nch; ++ch) {
    int tn[KSC];
#pragma unroll
    for (int ks = 0; ks < KSC; ++ks) tn[ks] = tab[(ch + 1 < nch ? ch + 1 : ch) * KSC + ks];
    if (ch + 1 < nch) issue_w(ch + 1);   // into the slot of chunk ch - 1 (behind the barrier that ended it)
    const u32x4* wb = Ws + (ch % RING) * WCHU + lane;
    const u32x4* xb = Xs + lanebase;
    auto rd = [&](int ks, u32x4 (&bq)[NP], u32x4 (&aq)[NP][FM]) {
#pragma unroll
      for (int q = 0; q < NP; ++q) bq[q] = xb[te[ks] + q * LOU];
#pragma unroll
      for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int i = 0; i < FM; ++i) aq[q][i] = wb[((ks * NP + q) * FM + i) * 64];
    };
#pragma unroll
    for (int h = 0; h < H; ++h) rd(h, bvA[h], aA[h]);
    __builtin_amdgcn_sched_barrier(0);
    if (ch > 0) {
#pragma unroll
      for (int h = 0; h < H2; ++h) mma(bvB[h], aB[h]);       // the held-back half of chunk ch - 1
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < H2; ++h) rd(H + h, bvB[h], aB[h]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < H; ++h) mma(bvA[h], aA[h]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < KSC; ++ks) te[ks] = tn[ks];
    wait_vm<0>();   // chunk ch + 1 (and, at ch = 0, the input tile's LDS-DMA) has landed; lgkmcnt(0): the table loads
    __builtin_amdgcn_s_barrier();
  }
  if (nch > 0) {
#pragma unroll
    for (int h = 0; h < H2; ++h) mma(bvB[h], aB[h]);
  }

  // ---- epilogue: 32x32 D tile: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ----
  const int t = t0 + wn * 32 + (lane & 31);
  if (t >= nt) return;
  const int hb = lane >> 5;
  auto unpack = [](uint2 w, float (&f)[4]) {
    f[0] = __builtin_bit_cast(float, w.x << 16); f[1] = __builtin_bit_cast(float, w.x & 0xffff0000u);
    f[2] = __builtin_bit_cast(float, w.y << 16); f[3] = __builtin_bit_cast(float, w.y & 0xffff0000u);
  };
  const bool masked = DX && P.eh != nullptr;
  const bool fmc = fmr && masked && P.ec != nullptr;   // feature-matching rows with a code plane (bl_edge.hip, bl_fm_code)

  if constexpr (DIR == DX_PR) {
    // ---- phases as rows in the order (channel bundle, phase, channel in bundle) (tap3_kernel's pr_order 1 form): stride 4 -- tile i
    // is bundle cb0 + i at the four phases of this lane's column; stride 2 -- a 32-row tile is two bundles at the two phases.  One
    // v_permlane32_swap per dword turns the lane's four half units into two whole units (32 contiguous bytes per lane).
    constexpr bool s4 = S == 4;
    static_assert(S == 2 || S == 4, "phases as rows at stride 2 or 4");
    const int tile0i = m0 >> 5;
    const long long LrowP = (long long)P.pr_Ly * 16;
    const long long tileP = (long long)(g * P.pr_cbg) * LrowP;
    const char* ehp = reinterpret_cast<const char*>(P.eh) + (long long)eb * P.CBy * LrowP + tileP;
    const char* elp = reinterpret_cast<const char*>(P.el) + (long long)eb * P.CBy * LrowP + tileP;
    const char* rhp = reinterpret_cast<const char*>(P.eh) + (long long)(b + P.bl_ref_off) * P.CBy * LrowP + tileP;
    const char* rlp = reinterpret_cast<const char*>(P.el) + (long long)(b + P.bl_ref_off) * P.CBy * LrowP + tileP;
    char* yhp = reinterpret_cast<char*>(P.yh) + (long long)b * P.CBy * LrowP + tileP;
    char* ylp = reinterpret_cast<char*>(P.yl) + (long long)b * P.CBy * LrowP + tileP;
    const int pos0 = s4 ? 4 * t + 2 * hb : 2 * t;
    const bool lv0 = pos0 < P.pr_Ly, lv1 = pos0 + 1 < P.pr_Ly;
    const unsigned poff = (unsigned)(lv0 ? pos0 : 0) * 16u;
    auto bund = [&](int i) { return s4 ? tile0i + i : 2 * (tile0i + i) + hb; };
    auto swap32 = [](unsigned& x, unsigned& y) {
      const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
      x = r[0]; y = r[1];
    };
    auto to_halves = [&](const u32x4 (&U)[2], uint2 (&Hh)[4]) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        unsigned x0 = U[j][0], x1 = U[j][1], y0 = U[j][2], y1 = U[j][3];
        swap32(x0, y0); swap32(x1, y1);
        Hh[j].x = x0; Hh[j].y = x1; Hh[2 + j].x = y0; Hh[2 + j].y = y1;
      }
    };
    auto to_units = [&](const uint2 (&Hh)[4], u32x4 (&U)[2]) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        unsigned x0 = Hh[j].x, x1 = Hh[j].y, y0 = Hh[2 + j].x, y1 = Hh[2 + j].y;
        swap32(x0, y0); swap32(x1, y1);
        U[j] = u32x4{x0, x1, y0, y1};
      }
    };
    auto ldu = [&](const char* base, int i, u32x4 (&U)[2]) {
      const int bd = bund(i);
      const char* q = base + (long long)(bd < P.pr_cbg ? bd : 0) * LrowP + poff;   // a bundle past the group's last: re-read, never stored
      U[0] = *reinterpret_cast<const u32x4*>(q);
      U[1] = *reinterpret_cast<const u32x4*>(q + (lv1 ? 16 : 0));
    };
    auto stu = [&](int i, const uint2 (&Hh)[4], char* base) {
      u32x4 U[2];
      to_units(Hh, U);
      const int bd = bund(i);
      char* q = base + (long long)bd * LrowP + poff;
      if (bd >= P.pr_cbg) return;
      if (lv0) *reinterpret_cast<u32x4*>(q) = U[0];
      if (lv1) *reinterpret_cast<u32x4*>(q + 16) = U[1];
    };
    const int tiles = (P.Mg - m0 + 31) >> 5;   // 32-row tiles of this block that exist (uniform)
    const char* ecp = reinterpret_cast<const char*>(P.ec) + (((long long)eb * P.CBy * LrowP + tileP) >> 1);
    u32x4 AU[FM][2];
    if (masked && (!fmr || fmc)) {
#pragma unroll
      for (int i = 0; i < FM; ++i) ldu(ehp, i < tiles ? i : 0, AU[i]);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if (i >= tiles) continue;
      uint2 AH[4], AL[4], RH[4], RL[4], OH[4], OL[4];
      unsigned CW[4] = {0u, 0u, 0u, 0u};
      if (masked && (!fmr || fmc)) {
        to_halves(AU[i], AH);
        if (fmc) {
          const int bd = bund(i);
          const char* q = ecp + (((long long)(bd < P.pr_cbg ? bd : 0) * LrowP + poff) >> 1);
          const uint2 c0 = *reinterpret_cast<const uint2*>(q);
          const uint2 c1 = *reinterpret_cast<const uint2*>(q + (lv1 ? 8 : 0));
          unsigned x0 = c0.x, y0 = c0.y, x1 = c1.x, y1 = c1.y;
          swap32(x0, y0); swap32(x1, y1);
          CW[0] = x0; CW[2] = y0; CW[1] = x1; CW[3] = y1;
        }
      } else if (masked) {
        u32x4 A2[2], L2[2], RH2[2], RL2[2];
        ldu(ehp, i, A2); ldu(elp, i, L2); ldu(rhp, i, RH2); ldu(rlp, i, RL2);
        to_halves(A2, AH); to_halves(L2, AL); to_halves(RH2, RH); to_halves(RL2, RL);
      }
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        float v[4], a0[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][4 * r4 + e];
        if (masked) {
          unpack(AH[r4], a0);
          if (fmc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const unsigned c = CW[r4] >> (8 * e);
              v[e] += fk1 * (float)((int)(c & 3u) - 1) - fk2 * (float)((int)((c >> 2) & 3u) - 1);
            }
          } else if (fmr) {
            float a1[4], r0[4], r1[4];
            unpack(AL[r4], a1); unpack(RH[r4], r0); unpack(RL[r4], r1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float av = a0[e] + a1[e], dv = av - (r0[e] + r1[e]);
              v[e] += fk1 * (float)((dv > 0.f) - (dv < 0.f)) - fk2 * (float)((av > 0.f) - (av < 0.f));
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= dlrelu(a0[e], P.emask_slope);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = lrelu(v[e], P.out_slope);
        }
        OH[r4].x = pack_bf16(v[0], v[1]); OH[r4].y = pack_bf16(v[2], v[3]);
        float hf[4];
        unpack(OH[r4], hf);
        OL[r4].x = pack_bf16(v[0] - hf[0], v[1] - hf[1]); OL[r4].y = pack_bf16(v[2] - hf[2], v[3] - hf[3]);
      }
      stu(i, OH, yhp);
      if (P.yl) stu(i, OL, ylp);
    }
    return;
  } else {
    // ---- row quad r4 of accumulator tile i: channels m0 + 32 i + 8 r4 + 4 hb .. +3, i.e. half hb of bundle (m0 >> 3) + 4 i + r4: one
    // 8-byte piece per lane.  The bundle row is block-uniform (scalar base), the lane's place in it ONE 32-bit byte offset; Mg is a
    // multiple of 8, so whether a quad exists is uniform too.
    const unsigned loff = (((unsigned)t * (unsigned)P.OS + (unsigned)oo) * 2u + (unsigned)hb) * 8u;   // bytes inside a bundle row
    const long long Lrow = (long long)P.Ly * 16;                                                  // bytes per bundle row
    const long long tile0 = ((long long)((g * P.Mg + m0) >> 3)) * Lrow;                           // this tile's first bundle row
    char* yhb = reinterpret_cast<char*>(P.yh) + (long long)b * P.CBy * Lrow + tile0;
    char* ylb = reinterpret_cast<char*>(P.yl) + (long long)b * P.CBy * Lrow + tile0;
    const int quads = (P.Mg - m0 + 7) >> 3;   // bundle rows of this tile that exist (uniform)
    if constexpr (DIR == FWD) {
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        float bz[4][4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const float4 bq = *reinterpret_cast<const float4*>(Bs + i * 32 + 8 * r4 + 4 * hb);
          bz[r4][0] = bq.x; bz[r4][1] = bq.y; bz[r4][2] = bq.z; bz[r4][3] = bq.w;
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int q = 4 * i + r4;
          if (q >= quads) continue;   // uniform
          const long long row = (long long)q * Lrow;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = lrelu(acc[i][4 * r4 + e] + bz[r4][e], P.out_slope);
          uint2 h;
          h.x = pack_bf16(v[0], v[1]); h.y = pack_bf16(v[2], v[3]);
          *reinterpret_cast<uint2*>(yhb + row + loff) = h;
          if (P.yl) {
            float hf[4];
            unpack(h, hf);
            uint2 l;
            l.x = pack_bf16(v[0] - hf[0], v[1] - hf[1]); l.y = pack_bf16(v[2] - hf[2], v[3] - hf[3]);
            *reinterpret_cast<uint2*>(ylb + row + loff) = l;
          }
        }
      }
    } else {
      // phase-scatter input gradient: no bias (the k-steps' sum + 0, as tap3_kernel adds its zero bias rows), then the mask and the
      // feature-matching term
      const char* ehb = reinterpret_cast<const char*>(P.eh) + (long long)eb * P.CBy * Lrow + tile0;
      const char* elb = reinterpret_cast<const char*>(P.el) + (long long)eb * P.CBy * Lrow + tile0;
      const char* rhb = reinterpret_cast<const char*>(P.eh) + (long long)(b + P.bl_ref_off) * P.CBy * Lrow + tile0;
      const char* rlb = reinterpret_cast<const char*>(P.el) + (long long)(b + P.bl_ref_off) * P.CBy * Lrow + tile0;
      const char* ecb = reinterpret_cast<const char*>(P.ec) + (((long long)eb * P.CBy * Lrow + tile0) >> 1);
      auto ld2 = [&](const char* base, long long row) { return *reinterpret_cast<const uint2*>(base + row + loff); };
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        uint2 ah[4], al[4], rh[4], rl[4];
        unsigned cw[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int q = 4 * i + r4;
          const long long row = (long long)(q < quads ? q : 0) * Lrow;   // uniform; a missing quad re-reads the tile's first row
          if (masked) {
            if constexpr (PREF) ah[r4] = pah[i][r4];
            else ah[r4] = ld2(ehb, row);
            if (fmc) cw[r4] = *reinterpret_cast<const unsigned*>(ecb + ((row + (long long)loff) >> 1));   // the half unit's four code bytes
            else if (fmr) { al[r4] = ld2(elb, row); rh[r4] = ld2(rhb, row); rl[r4] = ld2(rlb, row); }
          }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int q = 4 * i + r4;
          if (q >= quads) continue;   // uniform
          const long long row = (long long)q * Lrow;
          float v[4], a0[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[i][4 * r4 + e] + 0.f;
          if (masked) {
            unpack(ah[r4], a0);
            if (fmc) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const unsigned c = cw[r4] >> (8 * e);
                v[e] += fk1 * (float)((int)(c & 3u) - 1) - fk2 * (float)((int)((c >> 2) & 3u) - 1);
              }
            } else if (fmr) {
              float a1[4], r0[4], r1[4];
              unpack(al[r4], a1); unpack(rh[r4], r0); unpack(rl[r4], r1);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float av = a0[e] + a1[e], dv = av - (r0[e] + r1[e]);
                v[e] += fk1 * (float)((dv > 0.f) - (dv < 0.f)) - fk2 * (float)((av > 0.f) - (av < 0.f));
              }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= dlrelu(a0[e], P.emask_slope);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = lrelu(v[e], P.out_slope);
          }
          uint2 h;
          h.x = pack_bf16(v[0], v[1]); h.y = pack_bf16(v[2], v[3]);
          *reinterpret_cast<uint2*>(yhb + row + loff) = h;
          if (P.yl) {
            float hf[4];
            unpack(h, hf);
            uint2 l;
            l.x = pack_bf16(v[0] - hf[0], v[1] - hf[1]); l.y = pack_bf16(v[2] - hf[2], v[3] - hf[3]);
            *reinterpret_cast<uint2*>(ylb + row + loff) = l;
          }
        }
      }
    }
  }
}

template <int FM, int NP, int DIR, int S>
static int launch(const Tap3Args& a, int nblocks, size_t lds, hipStream_t st) {
  static LdsAttrOnce attr_once;
  auto kern = thin_bl_kernel<FM, NP, DIR, S>;
  {
    const hipError_t e = lds_attr_once(attr_once, reinterpret_cast<const void*>(kern));
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(thin_bl)");
  }
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), lds, st, a);
  EBEN_CHECK_LAUNCH("thin_bl_kernel");
  return EBEN_OK;
}

template <int NP, int DIR, int S>
static int launch_fm(int FM, const Tap3Args& a, int nblocks, size_t lds, hipStream_t st) {
  switch (FM) {
    case 1: return launch<1, NP, DIR, S>(a, nblocks, lds, st);
    case 2: return launch<2, NP, DIR, S>(a, nblocks, lds, st);
    case 3: return launch<3, NP, DIR, S>(a, nblocks, lds, st);
    default: return launch<4, NP, DIR, S>(a, nblocks, lds, st);
  }
}

enum { FORM_FWD_NP2_S2 = 1, FORM_FWD_NP1_S4, FORM_DX_PR_S2, FORM_DX_PR_S4, FORM_DX_PS };

}  // namespace thin

// The finished plan of a tap3_kernel launch and what the launch carries: the thin form that takes it, 0 when the launch is not one of the
// thin forms (tap3_kernel runs it).  Nothing here is per launch beyond a few comparisons of the plan.
int thin_bl_form(const Tap3Plan& p, const Tap3Call& k) {
  static const int enabled = getenv("EBEN_THIN_BL") ? atoi(getenv("EBEN_THIN_BL")) : 1;
  if (!enabled || !k.bl || p.big || k.reflect || k.in_mode || p.npw != p.npx || p.npw > 2) return 0;
  // one channel chunk in one input buffer, tap3_kernel's chunking and ring (the packed image and table are the plan's), <= 8 phases
  if (p.ncc != 1 || p.nxbuf != 1 || p.nph > 8 || p.FM < 1 || p.FM > 4 || p.BN != 128) return 0;
  if (p.KSC != thin::ksc_of(p.npw) || p.WCHU != p.KSC * p.npw * p.FM * 64) return 0;
  if (p.lds_bytes != (size_t)thin::RING * p.WCHU * 16 + ((size_t)p.CI_B * p.CSTRIDE * 16 + 16) * p.npx + (size_t)p.BM * 4) return 0;
  // the thin layers: <= 128 reduction channels and <= 256 rows per group
  if (p.Cg > 128 || p.Mg > 256) return 0;
  if (p.mode == 0 && k.pr_S == 0) {
    if (k.eh || k.res || k.accumulate || p.nph != 1) return 0;   // forward: bias + activation only
    if (p.S == 2 && p.npw == 2) return thin::FORM_FWD_NP2_S2;     // PQMF-band L1-L4
    if (p.S == 4 && p.npw == 1) return thin::FORM_FWD_NP1_S4;     // MelGAN L1-L2
    return 0;
  }
  if (p.npw != 1 || k.bias || k.res || k.accumulate) return 0;
  if (p.mode == 0) {   // phases as rows (the primed stride-1 layer)
    if (k.pr_order != 1 || p.S != 1 || p.nph != 1) return 0;
    if (k.pr_S == 2) return thin::FORM_DX_PR_S2;
    if (k.pr_S == 4) return thin::FORM_DX_PR_S4;
    return 0;
  }
  if (p.S != 1 || p.OS != 2 || p.nph != 2) return 0;   // phase scatter: the stride-2 input gradients that keep it (dilation 3)
  return thin::FORM_DX_PS;
}

int thin_bl_launch(const Tap3Plan& p, const Tap3Args& a, int form, int nblocks, hipStream_t st) {
  const size_t lds = p.lds_bytes;
  switch (form) {
    case thin::FORM_FWD_NP2_S2: return thin::launch_fm<2, thin::FWD, 2>(p.FM, a, nblocks, lds, st);
    case thin::FORM_FWD_NP1_S4: return thin::launch_fm<1, thin::FWD, 4>(p.FM, a, nblocks, lds, st);
    case thin::FORM_DX_PR_S2: return thin::launch_fm<1, thin::DX_PR, 2>(p.FM, a, nblocks, lds, st);
    case thin::FORM_DX_PR_S4: return thin::launch_fm<1, thin::DX_PR, 4>(p.FM, a, nblocks, lds, st);
    case thin::FORM_DX_PS: return thin::launch_fm<1, thin::DX_PS, 1>(p.FM, a, nblocks, lds, st);
    default: return fail(EBEN_EINVAL, "thin_bl: no thin form %d", form);
  }
}

}  // namespace eben
