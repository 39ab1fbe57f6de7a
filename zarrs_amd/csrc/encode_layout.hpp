// The host layout of the write path: everything the host decides about encoding chunks of one shape
// through one chain before anything touches the device. encode_layout() is a pure
// function of its arguments: no HIP call, no environment read (this header compiles without the ROCm
// headers), so it runs and is tested on a CPU (tests/test_encode_layout.py). write.cpp and store.cpp
// execute a layout: they allocate, copy and launch.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/zgpu.h"
#include "chain.hpp"
#include "common.hpp"
#include "plan_layout.hpp"

namespace zgpu {

#pragma GCC visibility push(hidden)
enum EncodePath : uint32_t {
  ENC_FIXED,        // gather into the destinations, checksums in place
  ENC_VAR,          // gather into slots, the stages over items, every chunk placed
  ENC_PACKBITS,     // `native` gathered, k_packbits, then `packed` over the packed chunks
  ENC_SHARD_FIXED,  // sharding_indexed over a fixed-size inner chain
  ENC_SHARD_VAR,    // sharding_indexed over a compressing inner chain
};

// One bytes->bytes codec of the chain (the fused innermost shuffle has no stage), in metadata order.
struct EncodeStage {
  StageKind kind;
  int at_start = 0;                      // checksum stages: the value leads the bytes
  uint64_t in_bound = 0, out_bound = 0;  // bytes in and out (exact on the fixed path)
  uint64_t lo = 0;  // ENC_FIXED: where the checksummed bytes start in a destination
  // materialising stages (strips_only(kind) false): the slot pool written, the launcher's parameters
  int pool = 0, level = 0;
  bool zstd_checksum = false;
  bool zlib = false, zlib_bounded = false;  // k_gzip_encode: a zlib stream, kept within zlib_bound
  uint32_t bl_comp = 0, bl_shuffle = 0, bl_typesize = 0;  // blosc: BL_COMP_*, 0 / 1 / 2, >= 1
  uint64_t bl_blocksize = 0;
};

struct EncodeLayout {
  EncodePath path = ENC_FIXED;
  const Chain *chain = nullptr;      // what it encodes: inside the chain it was made from (which must
  std::shared_ptr<const Chain> own;  // outlive it), or `own` (packbits' two chains)
  // the gather (ENC_FIXED, ENC_VAR): a fused innermost shuffle, the elements and bytes of one chunk,
  // (ENC_FIXED) 4 x the checksums located at the start
  bool shuffle = false;
  uint64_t nelem = 0, data_bytes = 0, data_off = 0;
  std::vector<EncodeStage> stages;
  // ENC_VAR slots: a chunk's bytes start `headroom` into its slot of `pitch` bytes, in n_pools pools
  // (ENC_SHARD_FIXED: the pitch of the inner chunks' temporary slots)
  uint64_t headroom = 0, pitch = 0;
  int n_pools = 0;
  // one chunk's encoded size (fixed: every chunk comes out with it) or its upper bound
  bool fixed = false;
  uint64_t size = 0;
  // sharding: inner chunks per shard along each axis and in all, elements of one, the inner chain's
  // layout and the index's (ENC_FIXED over 2 * n_inner uint64: its size, data_off and stages are the
  // index size, its checksums in front and the index checksum walk)
  uint64_t cps[ZG_MAXD] = {}, n_inner = 0, inner_n = 0;
  bool index_at_start = false, index_big_endian = false;
  std::shared_ptr<const EncodeLayout> inner, index;
  // packbits: [array->array codecs, bytes(native)] into slots of upitch bytes, packed into slots of
  // ppitch (direct: into the destinations), then [bytes(uint8), bytes->bytes codecs] over them
  std::shared_ptr<const EncodeLayout> native, packed;
  uint64_t packed_len = 0, upitch = 0, ppitch = 0;
  bool direct = false;
};
#pragma GCC visibility pop

// The layout of encoding chunks of chunk_shape through `c`, the chain after strip_value_codecs /
// retype_stripped (value codecs still in it are passed over; sizes are in the encoded element type).
// Throws ChainError for what the GPU does not encode: the array->bytes codec, a transpose of another
// rank, the bytes->bytes codecs in metadata order; for sharding_indexed: codecs around it, the index
// chain, the rank and divisibility of the shard shape, then the inner chain.
EncodeLayout encode_layout(const Chain &c, uint32_t nd, const uint64_t *chunk_shape);

// zgpu_chain_encoded_bound: the fixed size, the bounded size, for sharding_indexed every inner chunk at
// its bound plus the index (ShardingCodec::encoded_shard_bounded_size, sharding_codec.rs:924-945); -1 if
// unbounded. A size query, not an encode: numcodecs.bz2 is bounded here and value codecs keep the shape.
int64_t encoded_bound(const Chain &c, uint32_t nd, const uint64_t *chunk_shape);

}  // namespace zgpu
