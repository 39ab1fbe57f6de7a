// numcodecs.bz2 decode (bzip2 1.0.x streams, as libbz2's BZ2_bzDecompress reads them; zarrs:
// bytes_to_bytes/bz2/bz2_codec.rs -> bzip2::read::BzDecoder + read_to_end). The work unit is a block:
//
//   k_bz2_scan    one workgroup per item: "BZh1".."BZh9", then every bit offset is tested for the block
//                 magic 0x314159265359 and the end-of-stream magic 0x177245385090 -> candidate list
//   k_bz2_block   one wave per candidate (all of them, speculatively): header, code lengths, decode
//                 tables (libbz2's hbCreateDecodeTables), then the symbols: every lane decodes the code
//                 at its own bit of a 64-bit window, the wave walks the window's chain with readlanes
//                 (cut at the group's 50th symbol), applies the inverse MTF on a 256-entry list packed
//                 four per lane and expands RUNA / RUNB runs. Pass <false> only counts (end bit, nblock);
//                 pass <true>, after the chain is known, decodes the real blocks again and writes the
//                 BWT bytes into the region k_bz2_chain gave them
//   k_bz2_chain   one wave per item: bit 32 -> candidate -> its end bit -> ... -> end magic; candidates
//                 the chain does not reach (a magic inside a payload or in trailing bytes) are dropped;
//                 BWT regions by a running sum of nblock; the combined CRC
//   k_bz2_unbwt   1,024 threads per real block: stable counting sort (per-wave histograms in LDS, rank
//                 inside a wave by ballots) -> libbz2's tt[] (byte | successor << 8); sampled list
//                 ranking (<= 1,023 evenly spaced marks + the start; walk, order, walk again) writes the
//                 block's bytes before RLE1; the RLE1 parse gives the block's decoded length
//   k_bz2_place   per item: output offsets of its blocks, the decoded length, the item's {src, len}
//   k_bz2_emit    1,024 threads per real block: RLE1 inverse into the slot, CRC-32/BZIP2 of the bytes
//                 as they are written (per-thread registers merged by x^(8 len) mod P)
//
// RLE1 (four equal bytes, then a count byte 0..255) is a five-state automaton over the bytes (state:
// length 0..4 of the literal stretch so far; 4 = "the next byte is a count"), driven by "equals its
// predecessor". Each thread composes the transitions of its piece for all five start states; the start
// state of every piece then follows by applying 1,024 composed functions in turn. Stretches with no
// synchronisation point need no special case.
//
// Blocks with the randomised bit are CORRUPT_STREAM (a documented deviation).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.hpp"

namespace zgpu {
namespace {

constexpr uint64_t BZ_BLOCK_MAGIC = 0x314159265359ull, BZ_END_MAGIC = 0x177245385090ull;
constexpr uint32_t BZ_KIND_BLOCK = 0, BZ_KIND_END = 1;
constexpr uint32_t BZ_SKIP = 0x100u;  // item header status: nothing to do (failed earlier, fill, or done)
constexpr uint32_t BZ_MAX_SEL = 18002, BZ_MAX_ALPHA = 258, BZ_G = 50;
constexpr uint32_t BZ_POLY = 0x04C11DB7u;
constexpr uint32_t BZ_TMASK = 0xFFFFFu, BZ_MARK = 1u << 28;

struct Bz2Hdr {  // per item of a round (64 bytes)
  uint32_t ncand, nreal, level, status;
  uint64_t total;
  uint32_t pad[10];
};
struct Bz2Cand {  // 56 bytes
  uint64_t start;    // bit of the magic's first bit
  uint64_t end;      // first bit after the block's end-of-block symbol
  uint64_t tt_off;   // first entry of its region of the item's BWT scratch
  uint64_t out_off;  // first decoded byte in the item
  uint32_t nblock, orig, crc, status;
  uint32_t kind, dec_len;
};
static_assert(sizeof(Bz2Hdr) == 64 && sizeof(Bz2Cand) == 56, "scratch layout");

struct Bz2Lay {
  Bz2Hdr *hdr;
  Bz2Cand *cand;
  uint32_t *real;
  uint32_t *tt;
  uint8_t *u;
};
__device__ __forceinline__ Bz2Lay bz2_lay(const Bz2Scratch &S, uint32_t r) {
  uint8_t *b = S.base + (uint64_t)r * S.item_bytes;
  Bz2Lay L;
  L.hdr = (Bz2Hdr *)b;
  L.cand = (Bz2Cand *)(b + 64);
  L.real = (uint32_t *)(b + 64 + (uint64_t)S.cap * sizeof(Bz2Cand));
  L.tt = L.real + S.cap;
  L.u = (uint8_t *)(L.tt + S.tt_cap);
  return L;
}

// The round's work lists (S.lists: two counters, then round_items x cap entries each): list 0 the block
// candidates, list 1 the real blocks, as (item of the round) << 32 | record. The per-block kernels walk
// the list from entry blockIdx.x, so the work spreads over the whole chip; indexed by item x record the
// live workgroups sat at a fixed stride and landed on a fraction of the CUs.
__device__ __forceinline__ uint64_t *bz2_list(const Bz2Scratch &S, int which) {
  return (uint64_t *)(S.lists + 4) + (uint64_t)which * S.round_items * S.cap;
}

__device__ __forceinline__ uint32_t U(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bz2_scan(const ZgItem *items, uint32_t *status, uint32_t first,
                                                  Bz2Scratch S) {
  __shared__ uint32_t s_n;
  const uint32_t r = blockIdx.x, i = first + r, t = threadIdx.x;
  const Bz2Lay L = bz2_lay(S, r);
  const ZgItem it = items[i];
  if (status[i] || (it.flags & ZG_ITEM_FILL)) {
    if (t == 0) *L.hdr = Bz2Hdr{0, 0, 0, BZ_SKIP, 0, {}};
    return;
  }
  const uint8_t *src = (const uint8_t *)it.src;
  const uint64_t len = it.len;
  // the shortest stream: "BZh9", the end magic and the combined CRC
  bool ok = len >= 14;
  uint32_t level = 0;
  if (ok) {
    level = (uint32_t)src[3] - '0';
    ok = src[0] == 'B' && src[1] == 'Z' && src[2] == 'h' && level >= 1 && level <= 9;
  }
  if (!ok) {
    if (t == 0) {
      status[i] = ZG_CORRUPT_STREAM;
      *L.hdr = Bz2Hdr{0, 0, 0, BZ_SKIP, 0, {}};
    }
    return;
  }
  if (t == 0) s_n = 0;
  __syncthreads();
  for (uint64_t j = 4 + (uint64_t)t * 8; j < len; j += 256 * 8) {
    uint8_t b[15];
#pragma unroll
    for (int k = 0; k < 15; k++) b[k] = j + k < len ? src[j + k] : 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      uint64_t v = 0;  // 56 bits from byte j + k
#pragma unroll
      for (int q = 0; q < 7; q++) v = (v << 8) | b[k + q];
#pragma unroll
      for (int sh = 0; sh < 8; sh++) {
        const uint64_t m = (v >> (8 - sh)) & 0xFFFFFFFFFFFFull;
        if (m != BZ_BLOCK_MAGIC && m != BZ_END_MAGIC) continue;
        const uint64_t pos = (j + k) * 8 + sh;
        if (pos + 48 > len * 8) continue;
        const uint32_t c = atomicAdd(&s_n, 1u);
        if (c < S.cap) {
          Bz2Cand C{};
          C.start = pos;
          C.kind = m == BZ_BLOCK_MAGIC ? BZ_KIND_BLOCK : BZ_KIND_END;
          C.status = ZG_CORRUPT_STREAM;  // until k_bz2_block has decoded it
          L.cand[c] = C;
          if (m == BZ_BLOCK_MAGIC) bz2_list(S, 0)[atomicAdd(&S.lists[0], 1u)] = (uint64_t)r << 32 | c;
        }
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    // More magics than an item of this slot size is given records for: the item has outgrown its slot as
    // far as this stage can tell (the records grow with the slot, so a whole-shard stage's regrowing
    // reaches a slot whose records hold them)
    const bool over = s_n > S.cap;
    if (over) status[i] = ZG_DECODED_SIZE_MISMATCH;
    *L.hdr = Bz2Hdr{over ? 0u : s_n, 0, level, over ? BZ_SKIP : 0u, 0, {}};
  }
}

// ---------------------------------------------------------------------------------------------------
// The item's bits, MSB first, through two register windows of 64 big-endian words each (one coalesced
// load per window; a word is a readlane). Words are read aligned: the first and the last may reach up
// to three bytes outside the item, inside the same aligned word.
struct BitSrc {
  const uint32_t *base;
  uint32_t bit0;    // bit of the item's first byte inside word 0
  uint64_t last_w;  // last word that holds bytes of the item
  uint64_t chunk;   // cur = words [64 chunk, 64 chunk + 64), nxt the 64 after them
  uint32_t cur, nxt;
  uint32_t lane;
  __device__ __forceinline__ uint32_t load(uint64_t c) const {
    const uint64_t w = c * 64 + lane;
    return w <= last_w ? __builtin_bswap32(base[w]) : 0u;
  }
  __device__ __forceinline__ void init(const uint8_t *src, uint64_t len, uint32_t l) {
    base = (const uint32_t *)((uintptr_t)src & ~(uintptr_t)3);
    bit0 = (uint32_t)((uintptr_t)src & 3) * 8;
    last_w = (bit0 + len * 8 - 1) >> 5;
    lane = l;
    chunk = 0;
    cur = load(0);
    nxt = load(1);
  }
  __device__ __forceinline__ void ensure(uint64_t w) {  // w uniform; afterwards w .. w + 64 are readable
    const uint64_t c = w >> 6;
    if (c == chunk) return;
    if (c == chunk + 1) {
      cur = nxt;
    } else {
      cur = load(c);
    }
    chunk = c;
    nxt = load(c + 1);
  }
  __device__ __forceinline__ uint32_t word(uint64_t w) const {
    const uint32_t d = (uint32_t)(w - chunk * 64);
    return d < 64 ? U(__builtin_amdgcn_readlane(cur, (int)d)) : U(__builtin_amdgcn_readlane(nxt, (int)(d - 64)));
  }
  __device__ __forceinline__ uint32_t peek32(uint64_t p) {  // the 32 bits from bit p (uniform)
    const uint64_t a = bit0 + p, w = a >> 5;
    ensure(w);
    const uint32_t hi = word(w), lo = word(w + 1), sh = (uint32_t)a & 31;
    return sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
  }
};

struct BlockLds {
  uint8_t sel[BZ_MAX_SEL / 2];  // two selectors per byte
  uint8_t seq[256];
  uint8_t len[6][BZ_MAX_ALPHA];
  uint16_t perm[6][BZ_MAX_ALPHA];
  int32_t limit[6][24], base[6][24];
  uint32_t run[24];
  uint32_t minlen[6], maxlen[6];
};

template <bool WRITE>
__device__ __forceinline__ void bz2_block_one(BlockLds &D, uint32_t g, const ZgItem *items, uint32_t first,
                                              const Bz2Scratch &S) {
  const uint32_t lane = threadIdx.x;
  const uint64_t ent = bz2_list(S, WRITE ? 1 : 0)[g];
  const uint32_t r = (uint32_t)(ent >> 32), k = (uint32_t)ent;
  const Bz2Lay L = bz2_lay(S, r);
  const Bz2Hdr H = *L.hdr;
  if (H.status) return;
  uint32_t ci;
  if (WRITE) {
    if (k >= H.nreal) return;
    ci = L.real[k];
  } else {
    if (k >= H.ncand) return;
    ci = k;
  }
  Bz2Cand *C = &L.cand[ci];
  if (C->kind != BZ_KIND_BLOCK) return;
  const ZgItem it = items[first + r];
  const uint64_t end_bits = it.len * 8;
  uint32_t *tt = L.tt + (WRITE ? C->tt_off : 0);
  const uint64_t tt_room = WRITE ? S.tt_cap - C->tt_off : 0;
  BitSrc B;
  B.init((const uint8_t *)it.src, it.len, lane);
  uint64_t p = C->start + 48;
  auto get = [&](uint32_t n) -> uint32_t {
    const uint32_t v = B.peek32(p) >> (32 - n);
    p += n;
    return v;
  };
  const uint32_t crc = get(32);
  const uint32_t rnd = get(1);
  const uint32_t orig = get(24);
  bool bad = rnd != 0;
  // the symbol map
  const uint32_t used16 = get(16);
  uint32_t n_use = 0;
  for (uint32_t a = 0; a < 16; a++) {
    if (!((used16 >> (15 - a)) & 1)) continue;
    const uint32_t m = get(16);
    for (uint32_t b = 0; b < 16; b++)
      if ((m >> (15 - b)) & 1) {
        if (lane == 0) D.seq[n_use] = (uint8_t)(a * 16 + b);
        n_use++;
      }
  }
  const uint32_t alpha = n_use + 2;
  const uint32_t n_groups = get(3);
  uint32_t n_sel = get(15);
  bad = bad || n_use == 0 || n_groups < 2 || n_groups > 6 || n_sel < 1 || p > end_bits;
  if (bad) return;  // the record keeps CORRUPT_STREAM
  // selectors: unary MTF indices; those past 18,002 are read and dropped (libbz2 1.0.8)
  {
    uint32_t pos = 0x543210u;
    for (uint32_t a = 0; a < n_sel; a++) {
      const uint32_t j = (uint32_t)__clz((int)~B.peek32(p));  // leading ones
      if (j >= n_groups || p > end_bits) return;
      p += j + 1;
      if (a < BZ_MAX_SEL) {
        const uint32_t v = (pos >> (4 * j)) & 15, low = pos & ((1u << (4 * j)) - 1);
        pos = (pos & ~((1u << (4 * (j + 1))) - 1)) | (low << 4) | v;
        if (lane == 0) D.sel[a >> 1] = (uint8_t)((a & 1) ? (D.sel[a >> 1] | (v << 4)) : v);
      }
    }
    if (n_sel > BZ_MAX_SEL) n_sel = BZ_MAX_SEL;
  }
  // code lengths, delta coded
  for (uint32_t t = 0; t < n_groups; t++) {
    int curr = (int)get(5);
    for (uint32_t a = 0; a < alpha; a++) {
      for (;;) {
        if (curr < 1 || curr > 20 || p > end_bits) return;
        const uint32_t v = B.peek32(p);
        if (!(v >> 31)) {
          p += 1;
          break;
        }
        curr += ((v >> 30) & 1) ? -1 : 1;
        p += 2;
      }
      if (lane == 0) D.len[t][a] = (uint8_t)curr;
    }
  }
  if (p > end_bits) return;
  __syncthreads();
  // decode tables (hbCreateDecodeTables): perm = symbols by length then index, base, limit
  const uint64_t lt_mask = (1ull << lane) - 1;
  for (uint32_t t = 0; t < n_groups; t++) {
    if (lane < 24) D.run[lane] = 0;
    for (uint32_t a = lane; a < BZ_MAX_ALPHA; a += 64) D.perm[t][a] = 0xFFFF;
    __syncthreads();
    uint32_t mn = 32, mx = 0;
    for (uint32_t a = lane; a < alpha; a += 64) {
      const uint32_t l = D.len[t][a];
      mn = min(mn, l);
      mx = max(mx, l);
      atomicAdd(&D.run[l + 1], 1u);
    }
    for (int o = 32; o; o >>= 1) {
      mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
      mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    }
    __syncthreads();
    if (lane == 0) {
      D.minlen[t] = mn;
      D.maxlen[t] = mx;
      int32_t *base = D.base[t], *limit = D.limit[t];
      for (int a = 0; a < 23; a++) base[a] = (int32_t)D.run[a];
      for (int a = 1; a < 23; a++) base[a] += base[a - 1];
      for (int a = 0; a < 23; a++) D.run[a] = (uint32_t)base[a];  // first perm slot of each length
      for (int a = 0; a < 23; a++) limit[a] = 0;
      int32_t vec = 0;
      for (int a = (int)mn; a <= (int)mx; a++) {
        vec += base[a + 1] - base[a];
        limit[a] = vec - 1;
        vec <<= 1;
      }
      for (int a = (int)mn + 1; a <= (int)mx; a++) base[a] = ((limit[a - 1] + 1) << 1) - base[a];
    }
    __syncthreads();
    for (uint32_t a0 = 0; a0 < alpha; a0 += 64) {
      const uint32_t a = a0 + lane;
      const bool valid = a < alpha;
      const uint32_t l = valid ? D.len[t][a] : 0u;
      uint64_t eq = ~0ull;
      for (int b = 0; b < 5; b++) {
        const uint64_t bal = __ballot((l >> b) & 1);
        eq &= ((l >> b) & 1) ? bal : ~bal;
      }
      const uint32_t rank = (uint32_t)__popcll(eq & lt_mask);
      const uint32_t slot = D.run[l] + rank;
      __syncthreads();
      if (valid && slot < BZ_MAX_ALPHA) D.perm[t][slot] = (uint16_t)a;
      if (valid && rank == 0) D.run[l] += (uint32_t)__popcll(eq);
      __syncthreads();
    }
  }
  __syncthreads();
  // the symbols
  const uint32_t nblock_max = 100000u * H.level;
  const uint32_t eob = alpha - 1;
  // inverse-MTF list, four entries per lane (entry e: lane e / 4, bits 8 (e % 4) ..)
  uint32_t mtf = 0;
  for (int q = 3; q >= 0; q--) {
    const uint32_t e = lane * 4 + q;
    mtf = (mtf << 8) | (e < n_use ? D.seq[e] : 0u);
  }
  uint32_t nblock = 0, run = 0, run_n = 1;
  uint32_t group_no = 0, group_pos = 0, tb = 0, minlen = 1;
  bool done = false;
  while (!done) {
    if (group_pos == 0) {
      if (group_no >= n_sel) return;
      tb = U((D.sel[group_no >> 1] >> (4 * (group_no & 1))) & 15u);
      group_no++;
      group_pos = BZ_G;
      minlen = U(D.minlen[tb]);
    }
    if (p > end_bits) return;
    // every lane: the code that starts at bit p + lane
    uint32_t zn, sym;
    {
      const uint64_t a = B.bit0 + p, w = a >> 5;
      B.ensure(w);
      const uint32_t W0 = B.word(w), W1 = B.word(w + 1), W2 = B.word(w + 2), W3 = B.word(w + 3);
      const uint32_t off = ((uint32_t)a & 31) + lane, q = off >> 5, sh = off & 31;
      const uint32_t hi = q == 0 ? W0 : q == 1 ? W1 : W2, lo = q == 0 ? W1 : q == 1 ? W2 : W3;
      const uint32_t v = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
      const int32_t *limit = D.limit[tb], *base = D.base[tb];
      zn = minlen;
      int32_t zvec = 0;
      for (; zn <= 20; zn++) {
        zvec = (int32_t)(v >> (32 - zn));
        if (zvec <= limit[zn]) break;
      }
      sym = 0xFFFF;
      if (zn <= 20) {
        const int32_t x = zvec - base[zn];
        if (x >= 0 && x < (int32_t)BZ_MAX_ALPHA) sym = D.perm[tb][x];
      }
      if (sym >= alpha) zn = 0;  // no code here (an error only if the chain reaches this bit)
    }
    uint32_t pos = 0;
    while (pos < 64 && group_pos > 0) {
      const uint32_t z = U(__builtin_amdgcn_readlane(zn, (int)pos));
      const uint32_t s = U(__builtin_amdgcn_readlane(sym, (int)pos));
      if (z == 0) return;
      pos += z;
      group_pos--;
      if (s <= 1) {  // RUNA / RUNB: bijective base 2
        if (run_n >= 2u * 1024 * 1024) return;
        run += (s + 1) * run_n;
        run_n <<= 1;
        continue;
      }
      if (run) {
        if (nblock + run > nblock_max) return;
        if (WRITE) {
          const uint32_t uc = U(__builtin_amdgcn_readlane(mtf, 0)) & 0xff;
          for (uint32_t x = lane; x < run; x += 64)
            if (nblock + x < tt_room) tt[nblock + x] = uc;
        }
        nblock += run;
        run = 0;
        run_n = 1;
      }
      if (s == eob) {
        done = true;
        break;
      }
      if (nblock >= nblock_max) return;
      {
        const uint32_t idx = s - 1, q = idx >> 2, rr = idx & 3;
        const uint32_t wq = U(__builtin_amdgcn_readlane(mtf, (int)q));
        const uint32_t byte = (wq >> (8 * rr)) & 0xff;
        const uint32_t m = rr == 3 ? 0xFFFFFFFFu : (1u << (8 * (rr + 1))) - 1;
        if (q == 0) {
          if (lane == 0) mtf = (((mtf << 8) | byte) & m) | (mtf & ~m);
        } else {
          const uint32_t prev = (uint32_t)__shfl_up((int)mtf, 1, 64);
          const uint32_t shd = (mtf << 8) | (lane == 0 ? byte : prev >> 24);
          if (lane < q) mtf = shd;
          else if (lane == q) mtf = (shd & m) | (mtf & ~m);
        }
        if (WRITE && lane == 0 && nblock < tt_room) tt[nblock] = byte;
        nblock++;
      }
    }
    p += pos;
  }
  if (p > end_bits || orig >= nblock) return;
  if (!WRITE && lane == 0) {
    C->end = p;
    C->nblock = nblock;
    C->orig = orig;
    C->crc = crc;
    C->status = 0;
  }
}

// The per-block kernels run a bounded grid over the round's work list (entry g, g + gridDim.x, ...): the
// list's length is only known on the device, and a grid of its upper bound would be mostly empty.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_bz2_block(const ZgItem *items, uint32_t first, Bz2Scratch S) {
  __shared__ BlockLds D;
  const uint32_t n = S.lists[WRITE ? 1 : 0];
  for (uint32_t g = blockIdx.x; g < n; g += gridDim.x) {
    bz2_block_one<WRITE>(D, g, items, first, S);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bz2_chain(const ZgItem *items, uint32_t *status, uint32_t first,
                                                  uint32_t n_round, Bz2Scratch S) {
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  if (r >= n_round) return;
  const Bz2Lay L = bz2_lay(S, r);
  const Bz2Hdr H = *L.hdr;
  if (H.status) return;
  const ZgItem it = items[first + r];
  const uint8_t *src = (const uint8_t *)it.src;
  uint64_t cur = 32, tt_used = 0;
  uint32_t nreal = 0, comb = 0, st = ZG_CORRUPT_STREAM;
  for (uint32_t step = 0; step <= H.ncand; step++) {
    uint32_t f = 0xFFFFFFFFu;
    for (uint32_t c = lane; c < H.ncand; c += 64)
      if (L.cand[c].start == cur) f = c;
    for (int o = 32; o; o >>= 1) f = min(f, (uint32_t)__shfl_xor((int)f, o, 64));
    if (f == 0xFFFFFFFFu) break;  // the chain ends in nothing
    const Bz2Cand C = L.cand[f];
    if (C.kind == BZ_KIND_END) {
      if (cur + 80 > it.len * 8) break;
      uint32_t stored = 0;  // 32 bits from bit cur + 48
      const uint64_t b0 = (cur + 48) >> 3;
      const uint32_t sh = (uint32_t)(cur + 48) & 7;
      uint64_t v = 0;
      for (int q = 0; q < 5; q++) v = (v << 8) | (b0 + q < it.len ? src[b0 + q] : 0);
      stored = (uint32_t)(v >> (8 - sh));
      if (stored == comb) st = 0;
      break;
    }
    if (C.status) break;
    if (tt_used + C.nblock > S.tt_cap) {  // more BWT symbols than 1.25 x the slot: the item outgrew it
      st = ZG_DECODED_SIZE_MISMATCH;
      break;
    }
    if (lane == 0) {
      L.cand[f].tt_off = tt_used;
      L.real[nreal] = f;
      bz2_list(S, 1)[atomicAdd(&S.lists[1], 1u)] = (uint64_t)r << 32 | nreal;
    }
    tt_used += C.nblock;
    nreal++;
    comb = ((comb << 1) | (comb >> 31)) ^ C.crc;
    cur = C.end;
  }
  if (lane == 0) {
    L.hdr->nreal = st ? 0 : nreal;
    if (st) {
      L.hdr->status = BZ_SKIP;
      status[first + r] = st;
    } else if (S.blocks && nreal) {
      atomicAdd(S.blocks, (unsigned long long)nreal);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// RLE1 automaton. State: literals of the current stretch so far (0: fresh, 4: the next byte is a count).
__device__ __forceinline__ uint32_t rle1_step(uint32_t c, bool eq) {
  return c == 4 ? 0u : c == 0 ? 1u : eq ? c + 1 : 1u;
}

struct Rle1Lds {
  uint16_t f[1024];
  uint8_t st[1024];
  uint32_t len[1024];
  uint64_t off[1025];
  uint32_t fin;  // the state after the block's last byte
};

// Piece [a, b) of thread t, its start state and the decoded bytes before it (D.off[t]; D.off[1024]:
// the block's decoded length). All 1,024 threads call it.
__device__ __forceinline__ void rle1_scan(const uint8_t *u, uint32_t n, uint32_t t, Rle1Lds &D, uint32_t &a,
                                          uint32_t &b) {
  a = (uint32_t)((uint64_t)n * t >> 10);
  b = (uint32_t)((uint64_t)n * (t + 1) >> 10);
  uint32_t f = 0 | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12;
  for (uint32_t i = a; i < b; i++) {
    const bool eq = i > 0 && u[i] == u[i - 1];
    uint32_t g = 0;
#pragma unroll
    for (int s = 0; s < 5; s++) g |= rle1_step((f >> (3 * s)) & 7, eq) << (3 * s);
    f = g;
  }
  D.f[t] = (uint16_t)f;
  __syncthreads();
  if (t == 0) {
    uint32_t c = 0;
    for (uint32_t x = 0; x < 1024; x++) {
      D.st[x] = (uint8_t)c;
      c = (D.f[x] >> (3 * c)) & 7;
    }
    D.fin = c;
  }
  __syncthreads();
  uint32_t c = D.st[t], out = 0;
  for (uint32_t i = a; i < b; i++) {
    if (c == 4) {
      out += u[i];
      c = 0;
    } else {
      out++;
      c = rle1_step(c, i > 0 && u[i] == u[i - 1]);
    }
  }
  D.len[t] = out;
  __syncthreads();
  if (t == 0) {
    uint64_t o = 0;
    for (uint32_t x = 0; x < 1024; x++) {
      D.off[x] = o;
      o += D.len[x];
    }
    D.off[1024] = o;
  }
  __syncthreads();
}

struct UnbwtLds {
  uint32_t hist[16][256];
  uint32_t tot[256];
  uint32_t seg_len[1024], seg_nxt[1024], seg_off[1024];
  uint32_t ok, cycle;
};

__device__ __forceinline__ void bz2_unbwt_one(UnbwtLds &D, Rle1Lds &R, uint32_t g, const Bz2Scratch &S) {
  const uint32_t t = threadIdx.x;
  const uint64_t ent = bz2_list(S, 1)[g];
  const uint32_t r = (uint32_t)(ent >> 32), k = (uint32_t)ent;
  const Bz2Lay L = bz2_lay(S, r);
  if (L.hdr->status || k >= L.hdr->nreal) return;
  Bz2Cand *C = &L.cand[L.real[k]];
  const uint32_t n = C->nblock, orig = C->orig;
  uint32_t *tt = L.tt + C->tt_off;
  uint8_t *u = L.u + C->tt_off;
  const uint32_t wv = t >> 6, lane = t & 63;
  const uint32_t lo = (uint32_t)((uint64_t)n * wv >> 4), hi = (uint32_t)((uint64_t)n * (wv + 1) >> 4);
  for (uint32_t x = t; x < 16 * 256; x += 1024) (&D.hist[0][0])[x] = 0;
  __syncthreads();
  for (uint32_t i = lo + lane; i < hi; i += 64) atomicAdd(&D.hist[wv][tt[i] & 0xff], 1u);
  __syncthreads();
  if (t < 256) {
    uint32_t run = 0;
    for (int w = 0; w < 16; w++) {
      const uint32_t c = D.hist[w][t];
      D.hist[w][t] = run;
      run += c;
    }
    D.tot[t] = run;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int b = 0; b < 256; b++) {
      const uint32_t c = D.tot[b];
      D.tot[b] = run;
      run += c;
    }
  }
  __syncthreads();
  if (t < 256)
    for (int w = 0; w < 16; w++) D.hist[w][t] += D.tot[t];
  __syncthreads();
  // stable placement: entry i of byte b goes to the next free slot of b, in index order
  const uint64_t lt_mask = (1ull << lane) - 1;
  for (uint32_t i0 = lo; i0 < hi; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool valid = i < hi;
    const uint32_t key = valid ? (tt[i] & 0xff) : 256u;
    uint64_t eq = ~0ull;
    for (int b = 0; b < 9; b++) {
      const uint64_t bal = __ballot((key >> b) & 1);
      eq &= ((key >> b) & 1) ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(eq & lt_mask);
    uint32_t slot = 0;
    if (valid) slot = D.hist[wv][key] + rank;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) D.hist[wv][key] += (uint32_t)__popcll(eq);
    __builtin_amdgcn_wave_barrier();
    if (valid && slot < n) tt[slot] = (tt[slot] & 0xff) | (i << 8);  // only this thread writes entry slot
  }
  __threadfence_block();
  __syncthreads();
  // sampled list ranking of the walk p0 = T[orig], p(k+1) = T[p(k)]
  const uint32_t stride = max(1u, (n + 1022) / 1023);
  const uint32_t nm = (n + stride - 1) / stride;
  const uint32_t p0 = (tt[orig] >> 8) & BZ_TMASK;
  const bool special = p0 % stride != 0;
  const uint32_t nseg = nm + (special ? 1 : 0), sid = special ? nm : p0 / stride;
  __syncthreads();
  if (t < nm) tt[t * stride] |= BZ_MARK;
  if (t == 0 && special) tt[p0] |= BZ_MARK;
  if (t == 0) D.ok = 1;
  __threadfence_block();
  __syncthreads();
  const uint32_t start = t < nm ? t * stride : p0;
  if (t < nseg) {
    uint32_t cnt = 0, j = start, x = tt[j];
    for (;;) {
      cnt++;
      j = (x >> 8) & BZ_TMASK;
      if (j >= n || cnt > n) {
        D.ok = 0;
        j = start;
        break;
      }
      x = tt[j];
      if (x & BZ_MARK) break;
    }
    D.seg_len[t] = cnt;
    D.seg_nxt[t] = (special && j == p0) ? nm : j / stride;
  }
  __syncthreads();
  D.seg_off[t] = 0xFFFFFFFFu;
  __syncthreads();
  // The walk stays on the cycle of p0. Its length is n for the BWT of a primitive input; the BWT of an
  // input that is k copies of one string has k cycles of n / k, and libbz2 goes round p0's k times
  if (t == 0 && D.ok) {
    uint32_t id = sid, off = 0;
    bool ok = false;
    for (uint32_t c = 0; c < nseg; c++) {
      D.seg_off[id] = off;
      off += D.seg_len[id];
      id = D.seg_nxt[id];
      if (id == sid) {
        ok = true;
        break;
      }
    }
    D.ok = ok && off >= 1 && off <= n;
    D.cycle = off;
  }
  __syncthreads();
  if (!D.ok) {  // unreachable for a permutation; kept so that nothing is written on a broken invariant
    if (t == 0) {
      C->status = ZG_CORRUPT_STREAM;
      C->dec_len = 0;
    }
    return;
  }
  if (t < nseg && D.seg_off[t] != 0xFFFFFFFFu) {
    const uint32_t cyc = D.cycle;
    uint32_t o = D.seg_off[t], j = start;
    for (uint32_t c = D.seg_len[t]; c; c--) {
      const uint32_t x = tt[j];
      for (uint32_t q = o; q < n; q += cyc) u[q] = (uint8_t)x;
      o++;
      j = (x >> 8) & BZ_TMASK;
    }
  }
  __threadfence_block();
  __syncthreads();
  uint32_t a, b;
  rle1_scan(u, n, t, R, a, b);
  if (t == 0) {
    const uint64_t total = R.off[1024];
    C->dec_len = (uint32_t)total;  // at most 255 / 5 x 900,000
    // four equal bytes that end the block without their count: libbz2 reads the count past the block's
    // end and reports a data error (unRLE_obuf_to_output_FAST: nblock_used > save_nblock + 1)
    if (R.fin == 4) C->status = ZG_CORRUPT_STREAM;
  }
}

__global__ __launch_bounds__(1024) void k_bz2_unbwt(Bz2Scratch S) {
  __shared__ UnbwtLds D;
  __shared__ Rle1Lds R;
  const uint32_t n = S.lists[1];
  for (uint32_t g = blockIdx.x; g < n; g += gridDim.x) {
    bz2_unbwt_one(D, R, g, S);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bz2_place(ZgItem *items, uint32_t *status, uint32_t first, uint32_t n_round,
                                                  uint8_t *dst, uint64_t slot_bytes, Bz2Scratch S) {
  const uint32_t r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n_round) return;
  const Bz2Lay L = bz2_lay(S, r);
  if (L.hdr->status) return;
  const uint32_t i = first + r;
  uint64_t off = 0;
  bool bad = false;
  for (uint32_t k = 0; k < L.hdr->nreal; k++) {
    Bz2Cand *C = &L.cand[L.real[k]];
    bad = bad || C->status != 0;
    C->out_off = off;
    off += C->dec_len;
  }
  L.hdr->total = off;
  if (bad) {
    status[i] = ZG_CORRUPT_STREAM;
    L.hdr->status = BZ_SKIP;
  } else if (off > slot_bytes) {
    // the item stays on its input: the decoded length is only known to be larger. k_bz2_emit still runs
    // (it writes nothing past the slot) so that a block whose CRC fails makes it CORRUPT_STREAM, as
    // libbz2 reports it before the caller can compare sizes
    status[i] = ZG_DECODED_SIZE_MISMATCH;
  } else {
    items[i].src = (uint64_t)(dst + (uint64_t)i * slot_bytes);
    items[i].len = off;
  }
}

// x * y mod P, CRC-32/BZIP2's polynomial in the plain (MSB = highest power) representation
__device__ __forceinline__ uint32_t bz_mulmod(uint32_t x, uint32_t y) {
  uint32_t r = 0;
  for (int i = 31; i >= 0; i--) {
    r = (r << 1) ^ ((r >> 31) ? BZ_POLY : 0u);
    if ((x >> i) & 1) r ^= y;
  }
  return r;
}
__device__ __forceinline__ uint32_t bz_x8n(uint64_t nbytes) {  // x^(8 nbytes) mod P
  uint32_t res = 1, b = 0x100;
  while (nbytes) {
    if (nbytes & 1) res = bz_mulmod(res, b);
    b = bz_mulmod(b, b);
    nbytes >>= 1;
  }
  return res;
}

struct EmitLds {
  Rle1Lds R;
  uint32_t tab[256];
  uint32_t crc[1024];
  uint64_t len[1024];
};

__device__ __forceinline__ void bz2_emit_one(EmitLds &E, uint32_t g, uint32_t *status, uint32_t first, uint8_t *dst,
                                             uint64_t slot_bytes, const Bz2Scratch &S) {
  Rle1Lds &R = E.R;
  uint32_t *tab = E.tab, *s_crc = E.crc;
  uint64_t *s_len = E.len;
  const uint32_t t = threadIdx.x;
  const uint64_t ent = bz2_list(S, 1)[g];
  const uint32_t r = (uint32_t)(ent >> 32), k = (uint32_t)ent;
  const Bz2Lay L = bz2_lay(S, r);
  if (L.hdr->status || k >= L.hdr->nreal) return;
  const Bz2Cand *C = &L.cand[L.real[k]];
  const uint32_t n = C->nblock;
  const uint8_t *u = L.u + C->tt_off;
  const uint32_t i = first + r;
  uint8_t *out = dst + (uint64_t)i * slot_bytes;
  if (t < 256) {
    uint32_t c = t << 24;
    for (int q = 0; q < 8; q++) c = (c << 1) ^ ((c >> 31) ? BZ_POLY : 0u);
    tab[t] = c;
  }
  uint32_t a, b;
  rle1_scan(u, n, t, R, a, b);  // its barriers also cover tab
  uint64_t o = C->out_off + R.off[t];
  const uint64_t o0 = o;
  uint32_t c = R.st[t], crc = t == 0 ? 0xFFFFFFFFu : 0u;
  for (uint32_t x = a; x < b; x++) {
    const uint8_t v = u[x];
    if (c == 4) {
      const uint8_t pv = u[x - 1];  // x >= 4 here
      for (uint32_t q = 0; q < v; q++) {
        if (o < slot_bytes) out[o] = pv;
        o++;
        crc = (crc << 8) ^ tab[(crc >> 24) ^ pv];
      }
      c = 0;
    } else {
      if (o < slot_bytes) out[o] = v;
      o++;
      crc = (crc << 8) ^ tab[(crc >> 24) ^ v];
      c = rle1_step(c, x > 0 && v == u[x - 1]);
    }
  }
  s_crc[t] = crc;
  s_len[t] = o - o0;
  __syncthreads();
  for (uint32_t s = 1; s < 1024; s <<= 1) {
    if ((t & (2 * s - 1)) == 0) {
      const uint64_t l2 = s_len[t + s];
      s_crc[t] = bz_mulmod(s_crc[t], bz_x8n(l2)) ^ s_crc[t + s];
      s_len[t] += l2;
    }
    __syncthreads();
  }
  if (t == 0 && (s_crc[0] ^ 0xFFFFFFFFu) != C->crc) status[i] = ZG_CORRUPT_STREAM;
}

__global__ __launch_bounds__(1024) void k_bz2_emit(uint32_t *status, uint32_t first, uint8_t *dst,
                                                   uint64_t slot_bytes, Bz2Scratch S) {
  __shared__ EmitLds E;
  const uint32_t n = S.lists[1];
  for (uint32_t g = blockIdx.x; g < n; g += gridDim.x) {
    bz2_emit_one(E, g, status, first, dst, slot_bytes, S);
    __syncthreads();
  }
}

}  // namespace

uint64_t bz2_item_scratch_bytes(uint64_t slot_bytes, uint32_t &cap, uint64_t &tt_cap) {
  // RLE1 turns five BWT bytes into at least four decoded ones: an item that fits its slot has at most
  // 1.25 x slot_bytes BWT symbols (u32 each in tt, u8 each after the inverse BWT)
  tt_cap = (slot_bytes + slot_bytes / 4 + 3) & ~(uint64_t)3;
  // libbz2 fills a block with at least 99,981 symbols before it starts another; hand-made streams may not
  cap = (uint32_t)std::min<uint64_t>(32 + slot_bytes / 32768, 1u << 20);
  const uint64_t b = 64 + (uint64_t)cap * sizeof(Bz2Cand) + (uint64_t)cap * 4 + tt_cap * 4 + tt_cap;
  return (b + 255) & ~(uint64_t)255;
}

hipError_t launch_bz2(ZgItem *items, uint32_t *status, uint32_t n_items, uint8_t *dst, uint64_t slot_bytes,
                      const Bz2Scratch &S, hipStream_t s) {
  if (!n_items) return hipSuccess;
  if (!S.round_items || !S.base || !S.lists) return hipErrorInvalidValue;
  for (uint32_t first = 0; first < n_items; first += S.round_items) {
    const uint32_t nr = std::min(S.round_items, n_items - first);
    // the lists hold at most nr x cap entries; a block kernel's waves are long-lived, so its grid is a few
    // per CU and loops, as do the 1,024-thread kernels'
    const uint32_t bound = nr * S.cap, cus = device_cu_count();
    const uint32_t g64 = std::min(bound, cus * 16), g1024 = std::min(bound, cus * 4);
    hipError_t me = hipMemsetAsync(S.lists, 0, 16, s);
    if (me != hipSuccess) return me;
    hipLaunchKernelGGL(k_bz2_scan, dim3(nr), dim3(256), 0, s, items, status, first, S);
    hipLaunchKernelGGL(k_bz2_block<false>, dim3(g64), dim3(64), 0, s, items, first, S);
    hipLaunchKernelGGL(k_bz2_chain, dim3(nr), dim3(64), 0, s, items, status, first, nr, S);
    hipLaunchKernelGGL(k_bz2_block<true>, dim3(g64), dim3(64), 0, s, items, first, S);
    hipLaunchKernelGGL(k_bz2_unbwt, dim3(g1024), dim3(1024), 0, s, S);
    hipLaunchKernelGGL(k_bz2_place, dim3((nr + 63) / 64), dim3(64), 0, s, items, status, first, nr, dst, slot_bytes, S);
    hipLaunchKernelGGL(k_bz2_emit, dim3(g1024), dim3(1024), 0, s, status, first, dst, slot_bytes, S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace zgpu
