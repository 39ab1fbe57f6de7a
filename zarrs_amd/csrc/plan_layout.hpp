// The host layout of a fused decode plan: everything the host decides about a batch of chunk
// descriptors before anything touches the device -- the leaf work items and their geometry, the shard
// and middle-shard tables, the stage list and slot size, the scatter parameters and mode, and which
// stages may write straight into the output. plan_layout() is a pure function of its arguments: no HIP
// call, no environment read (this header compiles without the ROCm headers), so it runs and is tested
// on a CPU (tests/test_plan_layout.py). The device state built from a layout is zgpu_plan (plan.hpp).
#pragma once
#include <cstdint>
#include <optional>
#include <vector>

#include "../../include/zgpu.h"
#include "chain.hpp"
#include "common.hpp"

namespace zgpu {

#pragma GCC visibility push(hidden)
enum StageKind { ST_CRC32C, ST_GZIP, ST_ZSTD, ST_UNSHUFFLE, ST_BLOSC, ST_ADLER32, ST_FLETCHER32, ST_ZLIB, ST_BZ2 };
// the checksum stages strip 4 bytes in place; every other stage materialises its output in a slot pool
inline bool strips_only(StageKind k) { return k == ST_CRC32C || k == ST_ADLER32 || k == ST_FLETCHER32; }
inline StageKind checksum_stage(CodecKind k) {
  return k == CodecKind::Crc32c ? ST_CRC32C : k == CodecKind::Adler32 ? ST_ADLER32 : ST_FLETCHER32;
}
struct Stage {
  StageKind kind;
  int at_start = 0;          // checksum stages: the value leads the bytes
  uint32_t elementsize = 0;  // ST_UNSHUFFLE
  int pool = 0;              // destination slot pool for materialising stages
};
// The stage that decodes one bytes->bytes codec (pool left 0); nothing for any other codec.
std::optional<Stage> stage_for(const Codec &k);

// The switches the layout depends on, read from the environment once per plan creation
// (layout_knobs_from_env; tests and A/B runs flip them between plans of one process).
struct LayoutKnobs {
  uint32_t unshuffle_wide = 0;    // ZGPU_UNSHUFFLE_WIDE: 1 / 2 the 16-B unshuffle (scatter.hip), clamped to 0..2
  bool blosc_no_direct = false;   // ZGPU_BLOSC_NO_DIRECT set: blosc never writes into the output itself
  bool gzip_direct = true;        // ZGPU_GZIP_DIRECT=0 clears it: gzip never writes into the output itself
  bool blosc_no_partial = false;  // ZGPU_BLOSC_NO_PARTIAL set: blosc decodes every block of a partial item
};
LayoutKnobs layout_knobs_from_env();

struct PlanLayout {
  // leaf work items, their geometry (sel_start | sel_shape | out_start, 3 * nd each), plan-time
  // per-descriptor statuses, the sharded descriptors and (nested sharding) one record per intersecting
  // middle shard; ispec2: the middle shards' index
  std::vector<ZgItem> items;
  std::vector<uint64_t> geom;
  std::vector<uint32_t> item_desc_status;
  std::vector<ZgShard> shards;
  std::vector<ZgItem> mids;
  ZgIndexSpec ispec{}, ispec2{};
  // the leaf chain's bytes->bytes stages in decode order, and the slot pools they materialise into
  std::vector<Stage> stages;
  uint64_t slot_bytes = 0;
  int n_pools = 0;
  // the final fused stage. A tiled plan whose every item is a whole chunk of full, 16-B aligned tiles
  // scatters with k_scatter_tiled_p (tiled_persistent_params): its constants and the output element
  // offset of each item's origin
  ZgScatter scatter{};
  uint32_t scatter_mode = SCATTER_GENERIC;
  uint64_t scatter_units = 0;
  bool tiled_p = false;
  ZgTiledP tiled_q{};
  std::vector<uint64_t> origin;
  uint32_t first_path = SCATTER_GENERIC;  // what zgpu_plan_scatter_path reports before the first enqueue
  bool sharded = false, nested = false;
  const Chain *leaf = nullptr;    // inside the chain the layout was made from (which must outlive it)
  uint64_t alg_bytes_static = 0;  // decoded bytes written + (unsharded) encoded bytes + index bytes
  bool bl_direct = false;  // the blosc stage may write whole chunks straight into the output (BlDecode::dout)
  bool gz_direct = false;  // the gzip stage may write whole chunks straight into the output (gz)
  GzDirect gz{};
  // blosc as the last stage: per item the decoded byte range its selection needs ([0, max) for whole
  // chunks); blocks outside it are not decoded (blosc_decompress_bytes_partial). Empty: all of every item
  std::vector<uint64_t> bl_need;
  bool no_scatter = false;  // a stages-only layout: the bytes->bytes stages of a whole-shard predecode
};

// composed permutation of all array->array codecs: encoded axis a <-> decoded axis m[a]
void composed_axes(const Chain &c, uint32_t nd, uint32_t *m);
// ShardingIndex decode spec; throws ChainError for an index chain other than bytes (+ crc32c)
ZgIndexSpec index_spec(const Codec &sharding, uint64_t n_inner, bool validate);
#pragma GCC visibility pop

// The layout of a batch of n descriptors of an nd-dimensional array decoded by `top` into an output of
// out_shape. Throws ChainError for a chain the fused plan does not take; a descriptor that is wrong by
// itself gets its status in item_desc_status and no items.
PlanLayout plan_layout(const Chain &top, bool validate, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                       const uint64_t *out_shape, const LayoutKnobs &knobs);
// One stage over `items` (item j of descriptor j) with slots of slot_bytes (rounded up to 256), no scatter.
PlanLayout stages_only_layout(std::vector<ZgItem> items, Stage st, uint64_t slot_bytes);

}  // namespace zgpu
