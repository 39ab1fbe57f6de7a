// The zstd decoder's host launch policy (zstd_launch.hpp): pure functions, no device.
#include "zstd_launch.hpp"

#include <algorithm>
#include <cstdlib>

namespace zgpu {

ZstdKnobs zstd_knobs_from_env() {
  ZstdKnobs K;
  if (const char *e = std::getenv("ZGPU_ZSTD_XWIN")) K.xwin = std::atoi(e) < 0 ? -1 : std::atoi(e) != 0;
  if (const char *e = std::getenv("ZGPU_ZSTD_XPAR")) K.xpar = std::atoi(e) != 0;
  if (const char *e = std::getenv("ZGPU_ZSTD_XDENSE")) K.xdense = std::atoi(e) < 0 ? -1 : std::atoi(e) != 0;
  if (const char *e = std::getenv("ZGPU_ZSTD_FORCE_SERIAL")) K.force_serial = std::atoi(e) != 0;
  return K;
}

// The windowed workgroup executors for batches the wave executor would leave mostly idle (fewer than
// ZG_XWIN_MAX_WPC of its waves per CU: lone frames, per-chunk calls, C5's L1 and small levels); the wave
// executor for batches that fill the GPU with waves (C5's L0 halves, blosc-zstd), where the window
// executor's whole-CU workgroups measured slower beside the other lanes' entropy kernels (C5 100 vs
// 91-94 ms with it everywhere, profiles/r06/r06h_*). The threshold counts 3 waves per item, round 5's
// segment count.
static bool window_executors(uint64_t n_items, uint32_t cus, const ZstdKnobs &knobs) {
  return knobs.xwin >= 0 ? knobs.xwin != 0 : n_items * 3 < (uint64_t)cus * ZG_XWIN_MAX_WPC;
}

bool zstd_latency_possible(uint64_t n_items, uint64_t slot_bytes, uint32_t cus, const ZstdKnobs &knobs) {
  return window_executors(n_items, cus, knobs) && knobs.xpar && n_items * slot_bytes <= ZPAR_MAX_BYTES;
}

// Latency mode: the pointer-jumping rounds k_zstd_ext_round is launched for.
// Every hop of a reference chain leaves its window for an earlier window of the item (a
// cell is external only when its source lies before its window's start, exec_task), so a chain has
// at most as many hops as the item has windows. A latency-mode window ends at (a) its block's end:
// at most blk_cap of these; (b) the end of its workgroup's WSPAN range of the block: at most
// slot / WSPAN; (c) the end of a full sequence table (T = 1024 sequences of >= 3 bytes each): such
// a window starts either where the previous table ended, and then spans >= 3 T bytes (at most
// slot / (3 T) of these), or at its workgroup's range start (at most one per range: slot / WSPAN
// again). The W-cell limit never ends one: W > WSPAN. So
//   hops <= blk_cap + 2 slot / WSPAN + slot / (3 T) + 1,
// and pointer jumping resolves a chain of d hops in floor(log2 d) + 1 rounds (each round halves
// it); ceil(log2 hops) + 1 rounds are launched, at most ZEXT_ROUNDS (the largest latency batch,
// ZPAR_MAX_BYTES in one item, needs 17). A round after the last reference returns at once, and
// k_zstd_par_finish reads the last round's count: an item with a reference left reports an error.
static uint32_t ext_rounds(uint32_t blk_cap, uint64_t slot_bytes) {
  const uint64_t hops = (uint64_t)blk_cap + 2 * (slot_bytes / xwin::WSPAN) + slot_bytes / (3 * xwin::T) + 1;
  uint32_t rounds = 1;
  while (rounds < ZEXT_ROUNDS && (1ull << (rounds - 1)) < hops) rounds++;
  return rounds;
}

ZstdScratchSizes zstd_scratch_sizes(uint64_t n_items, uint64_t slot_bytes, uint32_t cus, const ZstdWants &wants) {
  ZstdScratchSizes S;
  S.blk_cap = (uint32_t)std::min<uint64_t>(slot_bytes / 32768 + 64, 1u << 20);
  // literals (<= the decoded size) + one Huffman table per block (HUF_TAB per >= 64 KiB of output on
  // typical frames; frames of many tiny Huffman blocks overflow it and take the serial decoder)
  S.lit_stride = (std::max<uint64_t>(slot_bytes + slot_bytes / 8, BLOCK_MAX + 64 + 2 * HUF_TAB) + 255) & ~(uint64_t)255;
  S.seq_cap = slot_bytes / 4 + 1024;  // sequences per item (each decodes >= 3 bytes; typical >= 8)
  // record slots: one per lane of k_zstd_lits' largest grid
  S.lit_rec_wgs = cus * ZG_LIT_GRID_PER_CU;
  S.blks = n_items * S.blk_cap * ZBLK_BYTES;
  S.norm = n_items * S.blk_cap * ZNORM * sizeof(int16_t);
  S.nblk = S.mode = S.ser_list = n_items * 4;
  S.lit = n_items * S.lit_stride;
  S.seq = n_items * S.seq_cap * 3 * sizeof(uint32_t);
  S.lit_rec = (uint64_t)S.lit_rec_wgs * LIT_THREADS * REC_SLOT;
  if (wants.alias) S.alias = n_items * 3 * ZALIAS * sizeof(uint64_t);
  if (wants.latency && zstd_latency_possible(n_items, slot_bytes, cus, wants.knobs)) {
    S.ext = 2 * n_items * slot_bytes * sizeof(uint32_t);  // two arrays of one u32 per decoded byte
    S.ext_cnt = ZEXT_ROUNDS * sizeof(unsigned long long);
  }
  return S;
}

ZstdLaunch zstd_launch_policy(uint64_t n_items, uint64_t slot_bytes, uint32_t cus, const ZstdCaps &caps,
                              const ZstdKnobs &knobs) {
  ZstdLaunch L;
  const uint32_t blk_cap = zstd_scratch_sizes(n_items, slot_bytes, cus, {}).blk_cap;
  // grids of the record-strided entropy kernels; k_zstd_lits: one resident wave of workgroups (CUs x
  // ZG_LIT_GRID_PER_CU of 256 lanes each); the sequence decoder: one of CUs x 4 SIMDs x ZG_BLK_WPE waves
  const uint64_t recs = n_items * blk_cap, g_cap = (uint64_t)cus * 16;
  L.grid = (uint32_t)std::min(recs, g_cap);
  L.lgrid = (uint32_t)std::min(recs, (uint64_t)cus * ZG_LIT_GRID_PER_CU);
  L.bgrid = (uint32_t)std::min(recs, std::max(g_cap, (uint64_t)cus * 4 * ZG_BLK_WPE));
  // the sequence decoder reads only the scan's block records and writes its own fields of them (and
  // the sequence scratch): with a side stream it runs beside the literal kernels
  L.fork = caps.side;
  L.lits_first = caps.lits_first && !L.fork;
  // literal-only blocks decoded straight into the slot: needs k_zstd_plan's output offsets before the
  // literal decoder, i.e. the sequence decoder on the same stream, and no aliases
  L.lit_direct = !L.fork && !caps.alias && !L.lits_first;
  L.rec_slots = L.lgrid <= caps.lit_rec_wgs;
  const bool win = window_executors(n_items, cus, knobs);
  L.xseg = win ? XSEG_WIN : XSEG;
  // the wave executor: xdense when the grid has many waves per CU
  const bool dense = knobs.xdense >= 0 ? knobs.xdense != 0 : n_items * L.xseg >= (uint64_t)cus * XDENSE_WAVES_PER_CU;
  const bool latency = caps.ext && zstd_latency_possible(n_items, slot_bytes, cus, knobs);
  L.executor = win ? (latency ? ZstdExecutor::LATENCY : ZstdExecutor::WINDOW)
                   : (dense ? ZstdExecutor::WAVE_DENSE : ZstdExecutor::WAVE_WIDE);
  if (L.executor == ZstdExecutor::LATENCY) {
    L.rounds = ext_rounds(blk_cap, slot_bytes);
    L.round_grid = (uint32_t)std::min((n_items * slot_bytes / 4 + 255) / 256, g_cap);
    L.persist_grid = cus;
  }
  // serial fallback: one wave per item, or (listed) a persistent grid of at most 4 waves per CU over the
  // compacted serial items, which a plan whose last execution had none does not launch
  L.serial = !caps.ser_list ? ZstdSerial::PER_ITEM : caps.launch_serial ? ZstdSerial::LISTED : ZstdSerial::NONE;
  L.serial_grid = (uint32_t)(L.serial == ZstdSerial::PER_ITEM ? n_items
                             : L.serial == ZstdSerial::LISTED ? std::min(n_items, (uint64_t)cus * 4) : 0);
  return L;
}

}  // namespace zgpu
