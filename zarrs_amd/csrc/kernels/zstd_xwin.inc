// The windowed zstd executor (k_zstd_exec_win), included once by zstd.hip after the block records,
// sym_eval and x_direct_block. Not a header: no include guard on purpose.
//
// LZ77 execution is a chain problem: every byte of a match equals the byte `offset` back, which may
// itself be a match byte. k_zstd_exec_item walks the sequences in order with one wave per executor
// segment, so a lone frame (per-chunk calls through a codec plugin) or a level of few large frames (C5's
// L1: 200 k sequences per 8 MiB chunk) runs on a handful of waves. Here one 512-thread workgroup owns a
// segment and decodes it in windows of up to 32 KiB, each window in parallel over its bytes:
//
//  1. the block's sequences covering the window are loaded (1024 at a time) and placed by a
//     workgroup prefix sum: sequence start, literal start, concrete offset (table in LDS);
//  2. every byte of the window becomes a 16-bit cell: a literal byte's value; for a match byte its
//     source s = M - off + ((p - M) mod off) (M the match start: the period reduction makes every
//     source precede its own match, so runs and overlapping copies are no chains), which is either
//     before the window (final: the value is loaded from the slot) or a pointer into the window;
//  3. pointer jumping in LDS (cell = cell[cell]) until every cell holds a value -- a chain inside a
//     window always ends at a literal or a far byte, and the jumps halve it every round: C5 frames
//     need 1.6-3.3 rounds per 32 KiB window on average and at most 7 (tools/lab/zstd_chain.cpp);
//  4. the window's bytes are stored to the slot with 16-B stores; the next window reads them back as
//     far sources (same workgroup: the barrier orders them).
//
// Bytes outside the window's compressed blocks (raw / rle / literal-only blocks) are copied by the
// workgroup or were written before the launch (k_zstd_direct, k_zstd_lits); executor segments are cut
// where no later match reaches back before the cut (k_zstd_plan), so a segment only reads itself.
//
// Latency mode (PAR = true: batches of a few frames, e.g. one chunk per call through a codec plugin):
// every window of every block gets a workgroup of its own, all at once. A cell whose chain leaves its
// window is not loaded (the byte may not exist yet) but becomes an external reference (32-bit cells:
// EXT | item position); k_zstd_ext_round then resolves the external references by pointer jumping
// over the whole output (ping-pong arrays, one launch per round: every hop of a chain leaves a window
// for an earlier one, so ceil(log2(an item's windows)) + 1 rounds; the bound on the windows is at the
// rounds rule in zstd_launch.cpp), and k_zstd_par_finish checks that no reference is left and the frame
// checksums.
// Reference behaviour: zarrs/src/array/codec/bytes_to_bytes/zstd/zstd_codec.rs:113-130 (libzstd
// ZSTD_decompress; RFC 8878 3.1.1.4 sequence execution).
namespace xwin {
// (THREADS, CELLS, W, T and WSPAN: zstd_params.hpp)
constexpr uint32_t NWAVE = THREADS / 64;
constexpr uint32_t E = (T + THREADS - 1) / THREADS;  // table entries per thread
constexpr uint32_t PER_LANE = CELLS / THREADS;  // cells per lane: one per row of its wave (64 or 32)
constexpr uint32_t ROWS = CELLS / 64;           // rows of 64 cells (a wave's row: one cell per lane)
#ifndef ZG_XWIN_G
#define ZG_XWIN_G 8
#endif
constexpr uint32_t XG = ZG_XWIN_G;              // rows per batch of global loads
constexpr int XR = 8;                           // pointer cells per lane and step of a round
static_assert(PER_LANE <= 64 && CELLS == NWAVE * 64 * PER_LANE && E <= 2, "cell ownership: a lane's cells in a u64 mask");

// cells: 16 bits (bit 15 a value in the low byte, else a window index); latency mode 32 bits (bit 31
// a value, bit 30 an external item position in the low 30 bits, else a window index)
template <bool PAR>
struct Cell {
  using T = uint16_t;
  static constexpr uint32_t RES = 0x8000u, EXT = 0u, DONE = 0x8000u;
};
template <>
struct Cell<true> {
  using T = uint32_t;
  static constexpr uint32_t RES = 0x80000000u, EXT = 0x40000000u, DONE = 0xC0000000u;
};
constexpr uint32_t EXT_NONE = 0xFFFFFFFFu;       // ext array: resolved
constexpr uint32_t WPB = (BLOCK_MAX + WSPAN - 1) / WSPAN;  // latency mode: workgroups per block

template <bool PAR>
struct alignas(16) Smem {
  typename Cell<PAR>::T cell[CELLS];
  uint32_t tS[T + 1], tL[T + 1], tO[T + 1];  // sequence start (item-relative), literal start, offset
  uint64_t rowbits[ROWS];  // bit b (>= 1): an entry starts at column b of the row
  uint16_t rowseq[ROWS + 2];
  uint32_t wsum[2][NWAVE];
  uint32_t nk, nS, nL;  // the entry holding the next window's start
  uint32_t rflag[3];    // pointer rounds: some cell of the round still holds a pointer (rotating)
  uint32_t skip;        // the task's item is not decoded here
  uint32_t err;
};

#ifdef ZG_XWIN_PROF
__device__ unsigned long long g_xwprof[16];  // clocks: table, rows, expand, rounds, output, classify | windows, rounds
#define XW_T(v) const uint64_t v = clock64()
#define XW_ADD(k, t) do { if (threadIdx.x == 0) atomicAdd(&g_xwprof[k], (unsigned long long)(clock64() - (t))); } while (0)
#define XW_CNT(k, n) do { if (threadIdx.x == 0) atomicAdd(&g_xwprof[k], (unsigned long long)(n)); } while (0)
#define XW_LANE_SUM(k, v) do { const uint32_t s_ = __builtin_amdgcn_readfirstlane(__reduce_add_sync(~0ull, (uint32_t)(v))); if ((threadIdx.x & 63) == 0) atomicAdd(&g_xwprof[k], (unsigned long long)s_); } while (0)
#else
#define XW_T(v)
#define XW_ADD(k, t)
#define XW_CNT(k, n)
#define XW_LANE_SUM(k, v)
#endif

// (d mod of) for d < 2^17, of >= 1: float reciprocal, one correction each way (branch-free)
__device__ __forceinline__ uint32_t mod_small(uint32_t d, uint32_t of) {
  const uint32_t q = (uint32_t)((float)d * __builtin_amdgcn_rcpf((float)of));
  int32_t r = (int32_t)d - (int32_t)(q * of);
  r += r < 0 ? (int32_t)of : 0;
  r -= r >= (int32_t)of ? (int32_t)of : 0;
  return (uint32_t)r;
}

// workgroup copy of n bytes (a raw / literal-only block the executor writes itself)
__device__ __forceinline__ void wg_copy(uint8_t *o, const uint8_t *s, uint32_t n) {
  for (uint32_t k = threadIdx.x; k < n; k += THREADS) o[k] = s[k];
}

}  // namespace xwin

namespace xwin {
// One task of the executor: segment sg of `item` (serial windows), or in latency mode the window range
// sg % WPB of block sg / WPB.
template <bool PAR>
__device__ __forceinline__ void exec_task(Smem<PAR> &S, uint32_t item, uint32_t sg, ZgItem *items, uint32_t *status,
                                          const ZBlk *blks, uint32_t blk_cap, const uint32_t *nblk,
                                          const uint32_t *zmode, uint8_t *dst, uint64_t slot_bytes,
                                          const uint8_t *lit_scratch, uint64_t lit_stride,
                                          const uint32_t *seq_scratch, uint64_t seq_cap, uint32_t *ext) {
  using C = Cell<PAR>;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // skip decided by one thread: another workgroup may write the item's status meanwhile, and a
  // workgroup whose threads disagreed would part at its barriers
  if (tid == 0) S.skip = zmode[item] != ZMODE_PARALLEL || status[item];
  __syncthreads();
  if (S.skip) return;
  uint8_t *out = dst + (uint64_t)item * slot_bytes;
  uint32_t *ext_item = PAR ? ext + (uint64_t)item * slot_bytes : nullptr;
  const ZBlk *B = blks + (uint64_t)item * blk_cap;
  const uint32_t nb = nblk[item];
  if (!nb) {
    if (!PAR && sg == 0 && tid == 0) {
      items[item].src = (uint64_t)out;
      items[item].len = 0;
    }
    return;
  }
  const uint8_t *in = (const uint8_t *)B[0].in_src;
  // this segment: blocks [b0, b1) between the sg-th and the next segment start (k_zstd_plan); latency
  // mode: block sg / WPB, its bytes [wi WSPAN, (wi + 1) WSPAN)
  uint32_t b0 = nb, b1 = nb, count = 0, wi = 0;
  if (PAR) {
    b0 = sg / WPB;
    b1 = b0 + 1;
    wi = sg % WPB;
  }
  for (uint32_t base = 0; !PAR && base < nb && count <= sg + 1; base += 64) {
    uint64_t m = __ballot(base + lane < nb && B[base + lane].seg);
    while (m && count <= sg + 1) {
      const uint32_t i = __builtin_ctzll(m);
      m &= m - 1;
      if (count == sg) b0 = base + i;
      else if (count == sg + 1) b1 = base + i;
      count++;
    }
  }
  if (b0 >= nb) return;  // fewer segments than workgroups for this item
  if (tid == 0) S.err = 0;
  __syncthreads();
  uint32_t err = 0;
  uint64_t fstart = B[b0].frame_off;
  uint64_t pos = B[b0].out_off;
  for (uint32_t bi = b0; bi < b1; bi++) {
    const ZBlk &R = B[bi];
    const uint32_t flags = R.flags, type = flags & 3;
    const uint64_t bstart = R.out_off;
    const uint32_t bsize = R.out_size;
    const uint64_t bend = bstart + bsize;
    if (flags & ZBF_FIRST) fstart = bstart;
    const uint32_t nseq = type == ZB_CMP ? R.nseq : 0u, regen = R.regen;
    if (PAR && wi && !(type == ZB_CMP && nseq && wi * WSPAN < bsize)) break;  // no window of this block
    if (x_direct_block(flags, nseq, bsize)) {  // in the slot already (k_zstd_direct / k_zstd_lits)
      if (type == ZB_CMP && regen != bsize) err = ZG_CORRUPT_STREAM;
    } else if (type == ZB_RAW) {
      wg_copy(out + bstart, in + R.in_off, bsize);
    } else if (type == ZB_RLE) {
      const uint8_t v = in[R.in_off];
      for (uint32_t k = tid; k < bsize; k += THREADS) out[bstart + k] = v;
    } else {
      const uint32_t ltype = (flags >> 2) & 3;
      const uint8_t *lsrc = ltype == 0 ? in + R.lit_off : lit_scratch + (uint64_t)item * lit_stride + R.lit_buf;
      if (nseq == 0) {
        if (regen != bsize) err = ZG_CORRUPT_STREAM;
        else wg_copy(out + bstart, lsrc, bsize);
      } else {
        const uint32_t *seqs = seq_scratch + ((uint64_t)item * seq_cap + R.seq_buf) * 3;
        const uint32_t ri0 = R.rep_in[0], ri1 = R.rep_in[1], ri2 = R.rep_in[2];
        // item-relative positions fit 32 bits (k_zstd_plan: < 0xFFFFFFF0)
        uint32_t k0 = 0, Sb = (uint32_t)bstart, Lb = 0, n = 0;
        uint32_t w0 = (uint32_t)bstart + (PAR ? wi * WSPAN : 0u);
        const uint32_t be = (uint32_t)bend;
        const uint32_t wend = PAR ? min<uint32_t>(be, w0 + WSPAN) : be;  // this workgroup's bytes end
        bool load = true;
        while (w0 < wend) {
          XW_T(t0);
          if (load) {
            // 1. table: entries k0 .. k0 + n - 1 (entry nseq: the trailing literals, no match)
            n = min<uint32_t>(T, nseq + 1 - k0);
            uint32_t ll[2] = {0, 0}, ml[2] = {0, 0}, of[2] = {0, 0};
#pragma unroll
            for (uint32_t h = 0; h < E; h++) {
              const uint32_t e = E * tid + h, idx = k0 + e;
              if (e < n && idx < nseq) {
                const uint32_t *q = seqs + (uint64_t)idx * 3;
                ll[h] = q[0];
                ml[h] = q[1];
                of[h] = sym_eval(q[2], ri0, ri1, ri2);
              }
            }
            const uint32_t a0 = ll[0] + ml[0], a1 = a0 + ll[1] + ml[1], c1 = ll[0] + ll[1];
            uint32_t ia = a1, ic = c1;  // wave inclusive scan
            for (int o = 1; o < 64; o <<= 1) {
              const uint32_t ta = __shfl_up(ia, o, 64), tc = __shfl_up(ic, o, 64);
              if ((int)lane >= o) { ia += ta; ic += tc; }
            }
            if (lane == 63) { S.wsum[0][wv] = ia; S.wsum[1][wv] = ic; }
            __syncthreads();
            uint32_t xa = ia - a1, xc = ic - c1;
            for (uint32_t w = 0; w < wv; w++) { xa += S.wsum[0][w]; xc += S.wsum[1][w]; }
#pragma unroll
            for (uint32_t h = 0; h < E; h++) {
              const uint32_t e = E * tid + h, idx = k0 + e;
              if (e >= n) break;
              // 64-bit sums: corrupt lengths must not wrap past the block end
              const uint64_t s0 = (uint64_t)Sb + xa + (h ? a0 : 0u), l0 = (uint64_t)Lb + xc + (h ? ll[0] : 0u);
              S.tS[e] = (uint32_t)min<uint64_t>(s0, be);
              S.tL[e] = (uint32_t)min<uint64_t>(l0, regen);
              S.tO[e] = of[h];
              if (idx < nseq) {
                const uint64_t send = s0 + ll[h] + ml[h], lend = l0 + ll[h], mstart = s0 + ll[h];
                if (send > be || lend > regen || of[h] == 0 || of[h] > mstart - fstart) err = ZG_CORRUPT_STREAM;
                if (e + 1 == n) { S.tS[n] = (uint32_t)min<uint64_t>(send, be); S.tL[n] = (uint32_t)min<uint64_t>(lend, regen); }
              } else {  // trailing literals: exactly the rest of the block
                if (l0 > regen || s0 > be || regen - l0 != be - s0) err = ZG_CORRUPT_STREAM;
                S.tS[n] = be;
                S.tL[n] = regen;
              }
            }
            if (__syncthreads_or(err != 0)) {
              if (err) S.err = err;
              break;
            }
            if (PAR && S.tS[n] <= w0) {  // latency mode: the table ends before this range, the next one
              k0 += n;
              Sb = S.tS[n];
              Lb = S.tL[n];
              __syncthreads();
              continue;
            }
          }
          XW_ADD(0, t0);
          XW_T(t1);
          // 2. the window [w0, w1) over cells from its 16-B aligned base wa
          const uint32_t tend = S.tS[n];
          const uint32_t wa = w0 - (uint32_t)((uintptr_t)(out + w0) & 15);
          const uint32_t w1 = min<uint32_t>(min<uint32_t>(wa + W, tend), wend);
          // rows of 64 cells: rowseq[r] = the entry holding the row's first position in the window
          // (clamped to [w0, w1 - 1]); rowbits[r] = the columns where a later entry starts
          for (uint32_t r = tid; r < ROWS; r += THREADS) S.rowbits[r] = 0;
          if (tid == 0) S.rflag[0] = 0;
          for (uint32_t r = tid; r <= ROWS; r += THREADS) {
            const uint32_t pr = min(max(wa + 64 * r, w0), w1 - 1);
            int32_t lo = 0, hi = (int32_t)n - 1;  // largest e with tS[e] <= pr
            while (lo < hi) {
              const int32_t mid = (lo + hi + 1) >> 1;
              if (S.tS[mid] <= pr) lo = mid;
              else hi = mid - 1;
            }
            S.rowseq[r] = (uint16_t)lo;
          }
          __syncthreads();
          for (uint32_t e = tid; e < n; e += THREADS) {
            const uint32_t st = S.tS[e];
            if (st > w0 && st < w1 && ((st - wa) & 63)) atomicOr(&S.rowbits[(st - wa) >> 6], 1ull << ((st - wa) & 63));
          }
          __syncthreads();
          XW_ADD(1, t1);
          XW_T(t2);
          // 3. cells: lane owns x = 64 (RW wv + i) + lane, i.e. column `lane` of rows RW wv + i (a wave's
          // rows are uniform: the entries overlapping a row are found once per row)
          uint64_t mask = 0;  // cells holding a pointer
          const uint64_t lmask = lane == 63 ? ~0ull : (2ull << lane) - 1;  // columns <= lane
#pragma unroll 1
          for (uint32_t g = 0; g < PER_LANE; g += XG) {
            XW_T(tb);
            // branch-free over the batch's rows: every LDS read of a row independent of the others
            uint32_t j[XG];
#pragma unroll
            for (uint32_t u = 0; u < XG; u++) {
              const uint32_t r = PER_LANE * wv + g + u;
              j[u] = S.rowseq[r] + (uint32_t)__builtin_popcountll(S.rowbits[r] & lmask);
            }
            uint32_t off[XG];
            // bit u: a literal load / a far load / a pointer cell / an external reference (latency mode)
            uint32_t ldl = 0, ldf = 0, pm = 0, pe = 0;
#pragma unroll
            for (uint32_t u = 0; u < XG; u++) {
              const uint32_t p = wa + 64 * (PER_LANE * wv + g + u) + lane;
              const uint32_t cS = S.tS[j[u]], cL = S.tL[j[u]], nL = S.tL[j[u] + 1], cO = S.tO[j[u]];
              const uint32_t M = cS + (nL - cL);
              const bool in = p >= w0 && p < w1, lit = p < M;
              const uint32_t src = M - cO + mod_small(p - M, max(cO, 1u));
              const bool far = !lit && src < w0;
              off[u] = lit ? cL + (p - cS) : far ? src : src - wa;
              ldl |= (uint32_t)(in && lit) << u;
              ldf |= (uint32_t)(in && far && !PAR) << u;
              pm |= (uint32_t)(in && !lit && !far) << u;
              pe |= (uint32_t)(in && far && PAR) << u;  // latency mode: an external reference
            }
            XW_ADD(5, tb);
            uint32_t v[XG];
#pragma unroll
            for (uint32_t u = 0; u < XG; u++) {
              const uint8_t *a = (ldl >> u & 1) ? lsrc + off[u] : out + ((ldf >> u & 1) ? off[u] : 0u);
              v[u] = *a;
            }
#pragma unroll
            for (uint32_t u = 0; u < XG; u++) {
              const uint32_t x = 64 * (PER_LANE * wv + g + u) + lane;
              if ((ldl | ldf) >> u & 1) S.cell[x] = (typename C::T)(C::RES | v[u]);
              else if (pm >> u & 1) S.cell[x] = (typename C::T)off[u];
              else if (PAR && (pe >> u & 1)) S.cell[x] = (typename C::T)(C::EXT | off[u]);
            }
            mask |= (uint64_t)pm << g;
            XW_LANE_SUM(9, __builtin_popcount(ldl));
            XW_LANE_SUM(10, __builtin_popcount(ldf));
          }
          XW_LANE_SUM(8, __builtin_popcountll(mask));
          XW_ADD(2, t2);
          XW_T(t3);
          // 4. pointer jumping until every cell of the window holds its value
          const uint32_t rbase = 64 * PER_LANE * wv + lane;
          // rounds: a wave with pointer cells left raises the round's flag; one barrier per round (the
          // flag of round rr + 1 is cleared in round rr: its last reader passed round rr - 1's barrier)
          for (uint32_t rr = 0;; rr++) {
            if (tid == 0) S.rflag[(rr + 1) % 3] = 0;
            if (__ballot(mask != 0) && lane == 0) S.rflag[rr % 3] = 1;
            __syncthreads();
            if (!S.rflag[rr % 3]) break;
            XW_CNT(7, 1);
            XW_T(tr);
            uint64_t m = mask;
            while (m) {
              XW_CNT(11, 1);
              uint32_t xi[XR], bit[XR];
              bool ok[XR];
#pragma unroll
              for (int u = 0; u < XR; u++) {
                ok[u] = m != 0;
                bit[u] = ok[u] ? (uint32_t)__builtin_ctzll(m) : 0u;
                m &= m - 1;  // m == 0 stays 0
                xi[u] = rbase + 64 * bit[u];
              }
              // unconditional reads (cell 0 for unused slots): the XR reads of each level issue back to
              // back, one wait per level instead of one per cell
              typename C::T c[XR], q[XR];
#pragma unroll
              for (int u = 0; u < XR; u++) c[u] = S.cell[ok[u] ? xi[u] : 0u];
#pragma unroll
              for (int u = 0; u < XR; u++) q[u] = S.cell[ok[u] ? (uint32_t)(c[u] & 0x7FFF) : 0u];
#pragma unroll
              for (int u = 0; u < XR; u++)
                if (ok[u]) {
                  S.cell[xi[u]] = q[u];
                  if (q[u] & C::DONE) mask &= ~(1ull << bit[u]);
                }
            }
            XW_ADD(12, tr);
          }
          XW_ADD(3, t3);
          XW_T(t4);
          // 5. the window's bytes to the slot: 16-B chunks from wa (cells 16 c .. 16 c + 15)
          const uint32_t nch = (w1 - wa + 15) >> 4;
          for (uint32_t ch = tid; ch < nch; ch += THREADS) {
            uint4 r;
            const uint32_t p = wa + 16 * ch;
            if constexpr (!PAR) {
              const uint4 *cp = (const uint4 *)&S.cell[16 * ch];
              const uint4 a = cp[0], b = cp[1];
              const uint32_t sel = 0x06040200u;
              r = make_uint4(__builtin_amdgcn_perm(a.y, a.x, sel), __builtin_amdgcn_perm(a.w, a.z, sel),
                             __builtin_amdgcn_perm(b.y, b.x, sel), __builtin_amdgcn_perm(b.w, b.z, sel));
            } else {
              // low bytes of 16 32-bit cells; external references to the ext array
              const uint4 *cp = (const uint4 *)&S.cell[16 * ch];
              uint32_t rw[4];
#pragma unroll
              for (int k = 0; k < 4; k++) {
                const uint4 c4 = cp[k];
                rw[k] = (c4.x & 0xFFu) | ((c4.y & 0xFFu) << 8) | ((c4.z & 0xFFu) << 16) | ((c4.w & 0xFFu) << 24);
                const uint32_t cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                  const uint32_t q = p + 4 * k + t;
                  if ((cc[t] & C::DONE) == C::EXT && q >= w0 && q < w1) ext_item[q] = cc[t] & 0x3FFFFFFFu;
                }
              }
              r = make_uint4(rw[0], rw[1], rw[2], rw[3]);
            }
            if (p >= w0 && p + 16 <= w1) {
              *(uint4 *)(out + p) = r;
            } else {
              const uint32_t rw[4] = {r.x, r.y, r.z, r.w};
              for (uint32_t k = 0; k < 16; k++)
                if (p + k >= w0 && p + k < w1) out[p + k] = (uint8_t)(rw[k >> 2] >> (8 * (k & 3)));
            }
          }
          // 6. the next window: the same table while it reaches the block end or a whole window past
          // w1, else a table from the entry holding w1 (the last entry's end: the entry after it)
          load = w1 < be && tend != be && tend - w1 < W;
          if (load) {
#pragma unroll
            for (uint32_t h = 0; h < E; h++) {
              const uint32_t e = E * tid + h;
              if (e < n && S.tS[e] <= w1 && (w1 < S.tS[e + 1] || e + 1 == n)) {
                const bool past = w1 >= S.tS[e + 1];  // w1 == the table end: the next entry
                S.nk = k0 + e + (past ? 1u : 0u);
                S.nS = past ? S.tS[e + 1] : S.tS[e];
                S.nL = past ? S.tL[e + 1] : S.tL[e];
              }
            }
          }
          __syncthreads();  // window stores before the next window's far loads; nk/nS/nL written
          if (load) {
            k0 = S.nk;
            Sb = S.nS;
            Lb = S.nL;
          }
          w0 = w1;
          __syncthreads();  // everyone has read the table, the rows and nk before they are rewritten
          XW_ADD(4, t4);
          XW_CNT(6, 1);
        }
      }
    }
    if (__syncthreads_or(err != 0)) {
      if (err) S.err = err;
      break;
    }
    if (S.err) break;
    pos = bend;
    if (!PAR && (flags & ZBF_LAST) && (flags & ZBF_CK)) {
      if (wv == 0) {
        const uint64_t h = xxh64(out + fstart, bend - fstart);
        if (lane == 0 && (uint32_t)h != R.ck) S.err = ZG_CORRUPT_STREAM;
      }
      __syncthreads();
      if (S.err) break;
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (S.err) {
      status[item] = S.err;
    } else if (!PAR && b1 == nb) {  // the last segment
      items[item].src = (uint64_t)out;
      items[item].len = pos;
    }
  }
}
}  // namespace xwin

// Serial windows: xseg workgroups per item, segment-major (XCD balance). Latency mode: a persistent
// grid over the tasks (item, block record < the batch's largest block count, window range); `xseg`
// then carries the batch's item count.
template <bool PAR>
__global__ __launch_bounds__(xwin::THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_zstd_exec_win(
    ZgItem *items, uint32_t *status, const ZBlk *blks, uint32_t blk_cap, const uint32_t *nblk, const uint32_t *zmode,
    uint8_t *dst, uint64_t slot_bytes, const uint8_t *lit_scratch, uint64_t lit_stride, const uint32_t *seq_scratch,
    uint64_t seq_cap, uint32_t xseg, uint32_t *ext, const unsigned long long *max_nblk) {
  __shared__ xwin::Smem<PAR> S;
  if constexpr (!PAR) {
    const uint32_t n_items = gridDim.x / xseg;
    xwin::exec_task<PAR>(S, blockIdx.x % n_items, blockIdx.x / n_items, items, status, blks, blk_cap, nblk, zmode, dst,
                         slot_bytes, lit_scratch, lit_stride, seq_scratch, seq_cap, ext);
  } else {
    const uint32_t n_items = xseg;
    const uint64_t nbm = max_nblk ? min<uint64_t>(blk_cap, *max_nblk) : blk_cap;
    const uint64_t tasks = (uint64_t)n_items * nbm * xwin::WPB;
    for (uint64_t t = blockIdx.x; t < tasks; t += gridDim.x) {
      xwin::exec_task<PAR>(S, (uint32_t)(t % n_items), (uint32_t)(t / n_items), items, status, blks, blk_cap, nblk,
                           zmode, dst, slot_bytes, lit_scratch, lit_stride, seq_scratch, seq_cap, ext);
      __syncthreads();
    }
  }
}

// Latency mode, external references: one pointer-jumping round over the batch's ext array (ea -> eb;
// EXT_NONE = resolved). A reference to a resolved position takes its byte and is resolved; any other
// jumps to that position's reference. cnt: references left after the round (the next round returns at
// once on 0). Four positions per thread (slot_bytes is a multiple of 256: one item).
__global__ __launch_bounds__(256) void k_zstd_ext_round(const uint32_t *ea, uint32_t *eb, uint8_t *dst,
                                                        uint64_t slot_bytes, uint64_t total,
                                                        const unsigned long long *cnt_prev,
                                                        unsigned long long *cnt) {
  using xwin::EXT_NONE;
  if (cnt_prev && *cnt_prev == 0) return;
  uint32_t left = 0;
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; 4 * q < total; q += (uint64_t)gridDim.x * 256) {
    const uint64_t p = 4 * q;
    const uint4 e = *(const uint4 *)(ea + p);
    uint32_t o[4] = {e.x, e.y, e.z, e.w};
    if ((e.x & e.y & e.z & e.w) != EXT_NONE) {
      const uint64_t base = p / slot_bytes * slot_bytes;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (o[k] == EXT_NONE) continue;
        const uint32_t t = ea[base + o[k]];
        if (t == EXT_NONE) {
          dst[p + k] = dst[base + o[k]];
          o[k] = EXT_NONE;
        } else {
          o[k] = t;
          left++;
        }
      }
    }
    *(uint4 *)(eb + p) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  const uint32_t w = __builtin_amdgcn_readfirstlane(__reduce_add_sync(~0ull, left));
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(cnt, (unsigned long long)w);
}

// Latency mode, last step: frame checksums over the resolved output and the items' decoded records
// (one wave per item). ext_fin / cnt_last: the ext array and the reference count the last round left;
// an item with a reference still in it (only when the count is not 0) is an error, never status 0
// over unresolved bytes. With the round count's bound (zstd_launch.cpp) no legal frame leaves a
// reference, so no test reaches that branch: it is a guard for a bound that a later change breaks.
// lat_count (nullable): the items finished here.
__global__ __launch_bounds__(64) void k_zstd_par_finish(ZgItem *items, uint32_t *status, const ZBlk *blks,
                                                        uint32_t blk_cap, const uint32_t *nblk,
                                                        const uint32_t *zmode, uint8_t *dst, uint64_t slot_bytes,
                                                        const uint32_t *ext_fin,
                                                        const unsigned long long *cnt_last,
                                                        unsigned long long *lat_count) {
  const uint32_t item = blockIdx.x;
  const int lane = lane_id();
  if (zmode[item] != ZMODE_PARALLEL || status[item]) return;
  uint8_t *out = dst + (uint64_t)item * slot_bytes;
  const ZBlk *B = blks + (uint64_t)item * blk_cap;
  const uint32_t nb = nblk[item];
  if (*cnt_last) {  // some item of the batch has references left: is it this one?
    const uint32_t *e = ext_fin + (uint64_t)item * slot_bytes;
    const uint64_t end = nb ? min<uint64_t>((uint64_t)U(B[nb - 1].out_off) + U(B[nb - 1].out_size), slot_bytes) : 0;
    bool left = false;
    for (uint64_t p = lane; p < end && !left; p += 64) left = e[p] != xwin::EXT_NONE;
    if (__ballot(left)) {
      if (lane == 0) status[item] = ZG_CORRUPT_STREAM;
      return;
    }
  }
  for (uint32_t base = 0; base < nb; base += 64) {
    uint64_t m = __ballot(base + lane < nb && (B[base + lane].flags & (ZBF_LAST | ZBF_CK)) == (ZBF_LAST | ZBF_CK));
    while (m) {
      const uint32_t bi = base + (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      const uint64_t fs = U(B[bi].frame_off), fe = (uint64_t)U(B[bi].out_off) + U(B[bi].out_size);
      const uint64_t h = xxh64(out + fs, fe - fs);
      if ((uint32_t)h != U(B[bi].ck)) {
        if (lane == 0) status[item] = ZG_CORRUPT_STREAM;
        return;
      }
    }
  }
  if (lane == 0) {
    items[item].src = (uint64_t)out;
    items[item].len = nb ? (uint64_t)B[nb - 1].out_off + B[nb - 1].out_size : 0;
    if (lat_count) atomicAdd(lat_count, 1ull);
  }
}
