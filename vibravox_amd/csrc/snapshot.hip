// Many tensors to one byte image and back: the device half of a training checkpoint (vibravox_amd/checkpoint.py).  `pack` gathers the
// tensors of a table into a flat image at 16-byte-aligned, ascending offsets, `unpack` scatters an image back into tensors that already
// exist.  Both copy bits -- 32-bit integers in 16-byte vectors or single bytes, never a float -- so NaN payloads, -0.0 and denormals
// arrive as they left.
//
//   pack_kernel     a block owns SNAP_BLOCK_BYTES consecutive bytes of one entry's SPAN: its bytes and the padding up to the next entry's
//                   offset (the last entry's: up to image_bytes), which is written as zeros, so that two images of one state are one
//                   sequence of bytes.  A block wholly inside its tensor whose source sits on the 16-byte grid loads its four vectors a
//                   lane and then stores them; every other block (a tail, a view off the grid, the padding) goes byte by byte.  For
//                   float32 entries the block counts the words whose exponent is all ones -- infinities and NaNs -- per wave, then per
//                   block in LDS, and adds a non-zero count to the entry's counter with one integer atomicAdd: integer sums, the same on
//                   every run.
//   unpack_kernel   the same two paths the other way, over the entries' own bytes and not one more.
//
// As for adam_kernel the table travels by value, SNAP_CHUNK entries a launch, and a launch is a flat list of blocks: bend[k] = blocks of
// the entries 0 .. k.  The host validates the whole table before the first launch.
#include <algorithm>
#include <vector>

#include "common.h"

namespace eben {
namespace {

constexpr int SNAP_CHUNK = 48;
constexpr int SNAP_THREADS = 256;
constexpr int SNAP_VECS = 4;                                        // 16-byte vectors a lane
constexpr int SNAP_BLOCK_BYTES = SNAP_THREADS * SNAP_VECS * 16;     // 16 KiB
constexpr unsigned EXP_MASK = 0x7f800000u;

struct SnapTable {
  EbenPackEntry t[SNAP_CHUNK];
  long long span[SNAP_CHUNK];   // pack: bytes from the entry's offset to the next entry's (the image's end); unpack: nbytes
  int bend[SNAP_CHUNK];
};

__device__ __forceinline__ int nonfinite_words(uint4 v) {
  return ((v.x & EXP_MASK) == EXP_MASK) + ((v.y & EXP_MASK) == EXP_MASK) + ((v.z & EXP_MASK) == EXP_MASK) + ((v.w & EXP_MASK) == EXP_MASK);
}

// the block's entry and the first byte of the entry it owns
__device__ __forceinline__ int snap_entry(const SnapTable& T, int n, long long* base) {
  int k = 0;
  while (k + 1 < n && (int)blockIdx.x >= T.bend[k]) ++k;   // block-uniform scan of <= 48 entries
  *base = (long long)((int)blockIdx.x - (k ? T.bend[k - 1] : 0)) * SNAP_BLOCK_BYTES;
  return k;
}

__global__ __launch_bounds__(SNAP_THREADS) void pack_kernel(const SnapTable T, int n, unsigned char* image, unsigned* nonfinite) {
  __shared__ int block_count;
  long long base;
  const int k = snap_entry(T, n, &base);
  const EbenPackEntry e = T.t[k];
  const unsigned char* src = static_cast<const unsigned char*>(e.tensor);
  unsigned char* dst = image + e.image_offset;   // on the 16-byte grid: the image and every offset are
  const bool count = e.kind == 1;
  const int t = threadIdx.x;
  int found = 0;
  if (count) {
    if (t == 0) block_count = 0;
    __syncthreads();
  }
  if ((reinterpret_cast<unsigned long long>(src) & 15ull) == 0 && base + SNAP_BLOCK_BYTES <= e.nbytes) {
    uint4 v[SNAP_VECS];
#pragma unroll
    for (int it = 0; it < SNAP_VECS; ++it) v[it] = *reinterpret_cast<const uint4*>(src + base + (long long)(it * SNAP_THREADS + t) * 16);
#pragma unroll
    for (int it = 0; it < SNAP_VECS; ++it) {
      *reinterpret_cast<uint4*>(dst + base + (long long)(it * SNAP_THREADS + t) * 16) = v[it];
      if (count) found += nonfinite_words(v[it]);
    }
  } else {
    const long long span = T.span[k];
    const long long end = base + SNAP_BLOCK_BYTES < span ? base + SNAP_BLOCK_BYTES : span;
    for (long long i = base + t; i < end; i += SNAP_THREADS) {
      unsigned char b = 0;
      if (i < e.nbytes) {
        b = src[i];
        // a float32's top byte (little endian: byte 3) and the byte below it hold the exponent; nbytes and base are multiples of 4
        if (count && (i & 3) == 3 && (b & 0x7f) == 0x7f && (src[i - 1] & 0x80)) ++found;
      }
      dst[i] = b;
    }
  }
  if (!count) return;   // block-uniform
  for (int d = 32; d; d >>= 1) found += __shfl_down(found, d);
  if ((t & 63) == 0 && found) atomicAdd(&block_count, found);
  __syncthreads();
  if (t == 0 && block_count) atomicAdd(nonfinite + e.reserved, (unsigned)block_count);   // reserved: the entry's place in the whole table
}

__global__ __launch_bounds__(SNAP_THREADS) void unpack_kernel(const SnapTable T, int n, const unsigned char* image) {
  long long base;
  const int k = snap_entry(T, n, &base);
  const EbenPackEntry e = T.t[k];
  unsigned char* dst = static_cast<unsigned char*>(e.tensor);
  const unsigned char* src = image + e.image_offset;
  const int t = threadIdx.x;
  if ((reinterpret_cast<unsigned long long>(dst) & 15ull) == 0 && base + SNAP_BLOCK_BYTES <= e.nbytes) {
    uint4 v[SNAP_VECS];
#pragma unroll
    for (int it = 0; it < SNAP_VECS; ++it) v[it] = *reinterpret_cast<const uint4*>(src + base + (long long)(it * SNAP_THREADS + t) * 16);
#pragma unroll
    for (int it = 0; it < SNAP_VECS; ++it) *reinterpret_cast<uint4*>(dst + base + (long long)(it * SNAP_THREADS + t) * 16) = v[it];
    return;
  }
  const long long end = base + SNAP_BLOCK_BYTES < e.nbytes ? base + SNAP_BLOCK_BYTES : e.nbytes;
  for (long long i = base + t; i < end; i += SNAP_THREADS) dst[i] = src[i];
}

inline long long snap_blocks(long long bytes) { return (bytes + SNAP_BLOCK_BYTES - 1) / SNAP_BLOCK_BYTES; }

// the rules both directions share; `ascending` (pack) also asks for the table's order to be the image's
int snap_validate(const char* what, const EbenPackEntry* table, int n, const void* image, long long image_bytes, bool ascending) {
  EBEN_REQUIRE(table && n > 0, "%s: a table of %d entries at %p", what, n, (const void*)table);
  EBEN_REQUIRE(image && (reinterpret_cast<uintptr_t>(image) & 15) == 0, "%s: the image at %p is null or off the 16-byte grid", what, image);
  EBEN_REQUIRE(image_bytes >= 0 && (image_bytes & 15) == 0, "%s: an image of %lld bytes (a non-negative multiple of 16)", what, image_bytes);
  for (int i = 0; i < n; ++i) {
    const EbenPackEntry& e = table[i];
    EBEN_REQUIRE(e.tensor, "%s: entry %d has a null tensor", what, i);
    EBEN_REQUIRE(e.kind == 0 || e.kind == 1, "%s: entry %d has the unknown kind %d", what, i, e.kind);
    EBEN_REQUIRE(e.nbytes >= 0, "%s: entry %d has %lld bytes", what, i, e.nbytes);
    EBEN_REQUIRE(e.kind == 0 || ((e.nbytes & 3) == 0 && (reinterpret_cast<uintptr_t>(e.tensor) & 3) == 0),
                 "%s: entry %d is float32 with %lld bytes at %p (multiples of 4)", what, i, e.nbytes, e.tensor);
    EBEN_REQUIRE(e.image_offset >= 0 && (e.image_offset & 15) == 0, "%s: entry %d starts at byte %lld, not a multiple of 16", what, i, e.image_offset);
    EBEN_REQUIRE(e.image_offset <= image_bytes && e.nbytes <= image_bytes - e.image_offset, "%s: entry %d holds the bytes [%lld, %lld) of an image of %lld",
                 what, i, e.image_offset, e.image_offset + e.nbytes, image_bytes);
    if (ascending && i > 0)
      EBEN_REQUIRE(e.image_offset >= table[i - 1].image_offset + table[i - 1].nbytes, "%s: entry %d at byte %lld starts before entry %d ends at %lld", what, i,
                   e.image_offset, i - 1, table[i - 1].image_offset + table[i - 1].nbytes);
  }
  if (!ascending) {
    std::vector<int> order;   // the entries that hold bytes: an empty one overlaps nothing, wherever it sits
    order.reserve(n);
    for (int i = 0; i < n; ++i)
      if (table[i].nbytes) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return table[a].image_offset < table[b].image_offset; });
    for (size_t j = 1; j < order.size(); ++j) {
      const EbenPackEntry &a = table[order[j - 1]], &b = table[order[j]];
      EBEN_REQUIRE(b.image_offset >= a.image_offset + a.nbytes, "%s: entries %d and %d overlap in the image", what, order[j - 1], order[j]);
    }
  }
  return EBEN_OK;
}

// the chunk [p0, p0 + cnt) as a launch table; false when its blocks do not fit a grid
bool snap_chunk(const EbenPackEntry* table, int n, int p0, int cnt, long long image_bytes, bool pack, SnapTable* T, long long* blocks_out) {
  long long blocks = 0;
  for (int i = 0; i < cnt; ++i) {
    const int g = p0 + i;
    T->t[i] = table[g];
    T->t[i].reserved = g;   // the entry's counter
    T->span[i] = pack ? (g + 1 < n ? table[g + 1].image_offset : image_bytes) - table[g].image_offset : table[g].nbytes;
    blocks += snap_blocks(T->span[i]);
    if (blocks > 0x7fffffffLL) return false;
    T->bend[i] = (int)blocks;
  }
  for (int i = cnt; i < SNAP_CHUNK; ++i) {
    T->t[i] = EbenPackEntry{nullptr, 0, 0, 0, 0};
    T->span[i] = 0;
    T->bend[i] = (int)blocks;
  }
  *blocks_out = blocks;
  return true;
}

}  // namespace
}  // namespace eben

using namespace eben;

extern "C" int eben_pack_plan(const EbenPackEntry* table, int n, long long* blocks, int* block_bytes) {
  EBEN_REQUIRE(n >= 0 && (table || n == 0), "pack_plan: a table of %d entries at %p", n, (const void*)table);
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    EBEN_REQUIRE(table[i].nbytes >= 0, "pack_plan: entry %d has %lld bytes", i, table[i].nbytes);
    const long long span = i + 1 < n ? table[i + 1].image_offset - table[i].image_offset : ((table[i].nbytes + 15) & ~15ll);
    EBEN_REQUIRE(span >= table[i].nbytes, "pack_plan: entry %d reaches past entry %d's offset", i, i + 1);
    total += snap_blocks(span);
  }
  if (blocks) *blocks = total;
  if (block_bytes) *block_bytes = SNAP_BLOCK_BYTES;
  return EBEN_OK;
}

extern "C" int eben_pack_tensors(const EbenPackEntry* table, int n, void* image, long long image_bytes, unsigned* nonfinite, void* stream) {
  const char* what = "pack_tensors";
  const int rc = snap_validate(what, table, n, image, image_bytes, true);
  if (rc != EBEN_OK) return rc;
  bool floats = false;
  for (int i = 0; i < n; ++i) floats = floats || table[i].kind == 1;
  EBEN_REQUIRE(!floats || (nonfinite && (reinterpret_cast<uintptr_t>(nonfinite) & 3) == 0), "%s: float32 entries need the counters, got %p", what,
               (void*)nonfinite);
  std::vector<SnapTable> chunks((n + SNAP_CHUNK - 1) / SNAP_CHUNK);
  std::vector<long long> blocks(chunks.size());
  for (size_t c = 0; c < chunks.size(); ++c) {
    const int p0 = (int)c * SNAP_CHUNK, cnt = n - p0 < SNAP_CHUNK ? n - p0 : SNAP_CHUNK;
    EBEN_REQUIRE(snap_chunk(table, n, p0, cnt, image_bytes, true, &chunks[c], &blocks[c]), "%s: the launch of entries %d ... is too large", what, p0);
  }
  hipStream_t s = as_stream(stream);
  if (nonfinite) {
    const hipError_t e = hipMemsetAsync(nonfinite, 0, sizeof(unsigned) * (size_t)n, s);
    if (e != hipSuccess) return hip_fail(e, "pack_tensors: zeroing the non-finite counts");
  }
  if (table[0].image_offset > 0) {   // what lies in front of the first entry is padding too
    const hipError_t e = hipMemsetAsync(image, 0, (size_t)table[0].image_offset, s);
    if (e != hipSuccess) return hip_fail(e, "pack_tensors: zeroing the image's head");
  }
  for (size_t c = 0; c < chunks.size(); ++c) {
    if (blocks[c] == 0) continue;
    const int cnt = n - (int)c * SNAP_CHUNK < SNAP_CHUNK ? n - (int)c * SNAP_CHUNK : SNAP_CHUNK;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)blocks[c]), dim3(SNAP_THREADS), 0, s, chunks[c], cnt, static_cast<unsigned char*>(image), nonfinite);
    EBEN_CHECK_LAUNCH("pack_kernel");
  }
  return EBEN_OK;
}

extern "C" int eben_unpack_tensors(const EbenPackEntry* table, int n, const void* image, long long image_bytes, void* stream) {
  const char* what = "unpack_tensors";
  const int rc = snap_validate(what, table, n, image, image_bytes, false);
  if (rc != EBEN_OK) return rc;
  std::vector<SnapTable> chunks((n + SNAP_CHUNK - 1) / SNAP_CHUNK);
  std::vector<long long> blocks(chunks.size());
  for (size_t c = 0; c < chunks.size(); ++c) {
    const int p0 = (int)c * SNAP_CHUNK, cnt = n - p0 < SNAP_CHUNK ? n - p0 : SNAP_CHUNK;
    EBEN_REQUIRE(snap_chunk(table, n, p0, cnt, image_bytes, false, &chunks[c], &blocks[c]), "%s: the launch of entries %d ... is too large", what, p0);
  }
  for (size_t c = 0; c < chunks.size(); ++c) {
    if (blocks[c] == 0) continue;
    const int cnt = n - (int)c * SNAP_CHUNK < SNAP_CHUNK ? n - (int)c * SNAP_CHUNK : SNAP_CHUNK;
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)blocks[c]), dim3(SNAP_THREADS), 0, as_stream(stream), chunks[c], cnt,
                       static_cast<const unsigned char*>(image));
    EBEN_CHECK_LAUNCH("unpack_kernel");
  }
  return EBEN_OK;
}
