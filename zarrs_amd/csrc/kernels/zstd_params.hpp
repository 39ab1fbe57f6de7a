// The constants of the zstd decode kernels (zstd.hip, zstd_xwin.inc) that the host's launch policy
// (../zstd_launch.hpp) sizes scratch and grids by. Plain values: no HIP header.
#pragma once
#include <cstdint>

namespace zgpu {

constexpr uint32_t BLOCK_MAX = 131072;
constexpr uint32_t MAX_HUF_LOG = 12;
// a block's Huffman decoding table in the literal scratch, right before its literals: 2^12 u16
// entries + a 16-B header holding the table log (0: invalid description)
constexpr uint32_t HUF_TAB = (1u << MAX_HUF_LOG) * 2 + 16;
// normalized-count scratch: per block record 3 tables x 64 int16 (counts of symbols 0..52; [62] the
// accuracy log, [63] the symbol count)
constexpr uint32_t ZNORM = 3 * 64;
constexpr uint32_t ZBLK_BYTES = 160;  // sizeof(ZBlk), the block record (zstd.hip asserts it)
constexpr uint32_t ZALIAS = 2;        // alias entries {src, off, len} per item (ZstdScratch::alias)
#ifndef ZG_BLK_WPE
#define ZG_BLK_WPE 6  // waves per SIMD k_zstd_blocks is compiled for
#endif
constexpr uint32_t LIT_THREADS = 256;
#ifndef ZG_LIT_GRID_PER_CU
#define ZG_LIT_GRID_PER_CU 4
#endif
// Record slot per lane: REC_OWN bytes of the lane's own chain (from its entry), then REC_RB bytes of
// a repair's true-chain prefix. A lane whose symbols do not fit decodes again (pass 2) instead.
constexpr uint32_t REC_OWN = 1024, REC_RB = 64, REC_SLOT = REC_OWN + REC_RB;

#ifndef ZG_XSEG
#define ZG_XSEG 12
#endif
// executor segments per item of the wave executor (at most). Round 5 measured 2, 3, 4 and 8 within 1 %
// with 3 best (profiles/r05/r05xs_zstd_exec_segment_major_xcd_ab.txt); with round 6's faster sequence
// decoder and the plan group the L0 executors end the C5 step, and more segments shorten them: C5 73.2
// (3), 72.5 (8), 70.8 (12), 71.3 (16), 103 (32) ms (profiles/r06/r06zfg_*); blosc-zstd's 2-block frames
// cut into 2 at most either way
constexpr uint32_t XSEG = ZG_XSEG;
#ifndef ZG_XSEG_WIN
#define ZG_XSEG_WIN 8
#endif
constexpr uint32_t XSEG_WIN = ZG_XSEG_WIN;  // executor segments per item (at most) for k_zstd_exec_win
// the window executor takes batches of fewer than this many of the wave executor's waves per CU
#ifndef ZG_XWIN_MAX_WPC
#define ZG_XWIN_MAX_WPC 4
#endif
// executor grids of at least this many waves (items x segments) per CU take xdense
#ifndef ZG_XDENSE_WPC
#define ZG_XDENSE_WPC 64
#endif
constexpr uint32_t XDENSE_WAVES_PER_CU = ZG_XDENSE_WPC;

namespace xwin {
#ifndef ZG_XWIN_THREADS
#define ZG_XWIN_THREADS 1024
#endif
constexpr uint32_t THREADS = ZG_XWIN_THREADS;
constexpr uint32_t CELLS = 32768;         // cells per window (u16: bit 15 resolved, else a 15-bit index)
constexpr uint32_t W = CELLS - 16;        // window span from its 16-B aligned base
constexpr uint32_t T = THREADS == 512 ? 768 : 1024;  // sequence table entries per load
constexpr uint32_t WSPAN = W - 16;        // latency mode: bytes of a block per workgroup
}  // namespace xwin
// latency mode: batches of at most this many decoded bytes (n_items x slot) get the ext arrays
constexpr uint64_t ZPAR_MAX_BYTES = 128ull << 20;
constexpr uint32_t ZEXT_ROUNDS = 24;  // round counters; the most rounds of k_zstd_ext_round

}  // namespace zgpu
