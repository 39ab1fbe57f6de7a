// The host's launch policy of the zstd decoder: how much scratch a batch gets and, per execution, every
// grid, the stream shape, the executor and the serial fallback's form. Plain values from plain values: no
// HIP call or header, no environment read outside zstd_knobs_from_env, so it runs and is tested on a CPU
// (tests/test_zstd_launch.py). launch_zstd enqueues what a ZstdLaunch says; DESIGN.md has the rules in a table.
#pragma once
#include <cstdint>

#include "kernels/zstd_params.hpp"

namespace zgpu {

// The switches tests drive, read from the environment when a plan's zstd scratch is sized and once per
// execution of a zstd or blosc stage (tests flip them between calls of one process).
struct ZstdKnobs {
  int xwin = -1;              // ZGPU_ZSTD_XWIN=0/1: the wave / the window executors for every batch
  bool xpar = true;           // ZGPU_ZSTD_XPAR=0 clears it: no latency mode
  int xdense = -1;            // ZGPU_ZSTD_XDENSE=0/1: the wave executor's wide / dense configuration
  bool force_serial = false;  // ZGPU_ZSTD_FORCE_SERIAL=1: every item on the serial one-wave decoder
};
ZstdKnobs zstd_knobs_from_env();

// Whether a batch of n_items slots of slot_bytes may take the latency mode on `cus` compute units: the
// window executors are on (forced, or the batch leaves the wave executor's grid sparse), the mode is not
// switched off, and the batch decodes to at most ZPAR_MAX_BYTES. Sizing and launch both ask this function.
bool zstd_latency_possible(uint64_t n_items, uint64_t slot_bytes, uint32_t cus, const ZstdKnobs &knobs);

// What the caller of zstd_scratch_sizes wants beside the pipeline's own buffers.
struct ZstdWants {
  bool alias = false;    // block aliases (the blosc stage, whose consumer reads the streams itself)
  bool latency = false;  // may take the latency mode (a plan's own zstd stage)
  ZstdKnobs knobs{};
};
// Bytes of the ZSTD_SCRATCH_BUFFERS buffers of ZstdScratch (0: not wanted) and the capacities they follow from.
constexpr int ZSTD_SCRATCH_BUFFERS = 11;
struct ZstdScratchSizes {
  uint32_t blk_cap = 0;      // block records per item
  uint64_t lit_stride = 0;   // literal scratch bytes per item
  uint64_t seq_cap = 0;      // sequences per item
  uint32_t lit_rec_wgs = 0;  // workgroups of k_zstd_lits the record slots serve
  uint64_t blks = 0, norm = 0, nblk = 0, mode = 0, lit = 0, seq = 0, ser_list = 0, lit_rec = 0, alias = 0, ext = 0, ext_cnt = 0;
};
ZstdScratchSizes zstd_scratch_sizes(uint64_t n_items, uint64_t slot_bytes, uint32_t cus, const ZstdWants &wants);

// What the caller's scratch and flags provide to one execution.
struct ZstdCaps {
  bool side = false;           // a side stream (and its two events) for the sequence decoder
  bool alias = false;          // ZstdScratch::alias
  bool lits_first = false;     // ZstdScratch::lits_first
  bool ext = false;            // the latency mode's ext arrays and round counters
  uint32_t lit_rec_wgs = 0;    // workgroups the literal record slots serve (0: none)
  bool ser_list = false;       // the compacted serial list and its count
  bool launch_serial = false;  // ZstdScratch::launch_serial
};
enum class ZstdExecutor : uint32_t { LATENCY, WINDOW, WAVE_DENSE, WAVE_WIDE };
enum class ZstdSerial : uint32_t { NONE, PER_ITEM, LISTED };
struct ZstdLaunch {
  uint32_t grid = 0, lgrid = 0, bgrid = 0;  // of k_zstd_huf and k_zstd_direct, k_zstd_lits, k_zstd_blocks
  bool fork = false;        // the sequence decoder on the side stream, beside the literal kernels
  bool lits_first = false;  // one stream: the literal kernels before the sequence decoder
  bool lit_direct = false;  // k_zstd_plan before the literal kernels, literal-only blocks into the slot
  bool rec_slots = false;   // k_zstd_lits gets the record slots
  uint32_t xseg = 0;        // executor segments per item (at most)
  ZstdExecutor executor = ZstdExecutor::WAVE_WIDE;
  // LATENCY: launches of k_zstd_ext_round, their grid, and k_zstd_exec_win<true>'s persistent grid
  uint32_t rounds = 0, round_grid = 0, persist_grid = 0;
  // the serial fallback: none, one wave per item, or a persistent grid over the compacted list (which
  // k_zstd_scan appends the serial items to unless PER_ITEM); serial_grid waves
  ZstdSerial serial = ZstdSerial::PER_ITEM;
  uint32_t serial_grid = 0;
};
ZstdLaunch zstd_launch_policy(uint64_t n_items, uint64_t slot_bytes, uint32_t cus, const ZstdCaps &caps,
                              const ZstdKnobs &knobs);

}  // namespace zgpu
