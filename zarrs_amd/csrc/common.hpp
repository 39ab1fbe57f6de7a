// Shared host/device definitions for the zgpu decode pipeline (gfx950).
//
// Device data layout (one "plan" = one batch of chunk descriptors):
//   Item[n_items]      leaf chunk work items (a plain chunk, or one inner chunk of a shard):
//                      current encoded byte range {src,len} that each b2b stage rewrites in place
//   geom[n_items][3*nd] u64: sel_start (leaf-chunk relative), sel_shape, out_start (output array)
//   status[n_items]    u32 per-item status (0 = ok; first error sticks, later stages skip)
//   Shard[n_shards]    sharded descriptors: encoded shard {ptr,len}; index decoded into
//   index[n_shards][n_inner*2] u64 (offset, nbytes) per inner chunk, C order of inner coords
#pragma once
#include <stddef.h>
#include <stdint.h>

#define ZG_MAXD 8

// item flags
#define ZG_ITEM_FILL 0x1u     // write the fill value (missing chunk / empty inner chunk)
#define ZG_ITEM_PARTIAL 0x2u  // partial-decoder path: crc32c strips without verifying
#define ZG_ITEM_SHARDED 0x4u  // src/len resolved on device from the shard index
#define ZG_ITEM_DIRECT 0x8u   // already written into the output by its last stage: the scatter skips it

struct ZgItem {
  uint64_t src;    // device address of the current encoded bytes
  uint64_t len;    // current byte length
  uint32_t desc;   // owning descriptor
  uint32_t flags;  // ZG_ITEM_*
  uint32_t shard;  // shard slot (sharded items)
  uint32_t inner;  // inner chunk linear index inside the shard
};

struct ZgShard {
  uint64_t ptr;  // device address of the encoded shard
  uint64_t len;
};

// Parameters of the final fused stage: bytes codec (endianness) + transpose(s) + scatter
// into the output subset (+ an innermost numcodecs.shuffle when it sits directly above bytes).
struct ZgScatter {
  uint32_t nd;
  uint32_t es;        // element size (bytes)
  uint32_t comp;      // component size for endianness swap
  uint32_t swap;      // 1: stored big-endian -> reverse each component
  uint32_t shuffle;   // 1: fused unshuffle with elementsize == es
  uint32_t tile_a;    // decoded axis that is innermost in the encoded layout (tiled kernel)
  uint32_t tile_b;    // tiled kernel: axis batched TJ slabs per block (smallest encoded stride
                      // among the other axes: adjacent slabs are adjacent encoded rows); ZG_MAXD = none
  uint32_t pad0;      // u16 unshuffle A/B (ZGPU_UNSHUFFLE_WIDE): 0 8-B plane loads, 1 / 2 16-B (nt / plain)
  uint64_t chunk_shape[ZG_MAXD];  // leaf decoded shape
  uint64_t enc_stride[ZG_MAXD];   // encoded linear stride (elements) of each decoded axis
  uint64_t out_stride[ZG_MAXD];   // output array C strides (elements)
  uint64_t nelem;                 // elements per leaf chunk
  uint8_t fill[16];
};

// k_gzip writing whole chunks straight into the output rows (the gzip stage last before a rows scatter
// with no swap / shuffle / transpose): an item whose selection is its whole chunk and whose output
// rows are 16-B aligned is decoded into the array, flagged ZG_ITEM_DIRECT, and the scatter skips it.
// Chunk byte p lives in row p >> lbs (C order over the leading axes) at column p & (2^lbs - 1).
struct GzDirect {
  uint8_t *dout;         // output array; nullptr: every item decodes into its slot
  const uint64_t *geom;  // per item: sel_start | sel_shape | out_start (ZG_MAXD-free: 3 * nd)
  uint64_t want;         // decoded bytes of a whole chunk
  uint64_t cshape[4];    // chunk shape
  uint64_t ostr[4];      // output byte stride of each axis
  uint32_t nd;           // <= 3 (axis 1 of a 3-d chunk has a power-of-two extent); byte strides < 4 GiB
  uint32_t lbs;          // log2 of the row bytes (chunk_shape[nd-1] * es, >= 16)
};

// What the host layout of a plan (plan_layout.hpp) shares with the launchers (kernels/launch.hpp), free
// of HIP: the scatter modes, the shard index spec, the persistent tiled scatter's constants. The three
// functions are defined in kernels/scatter.hip, next to the tile constants they share with the kernels.
namespace zgpu {

enum ScatterMode : uint32_t { SCATTER_ROWS = 0, SCATTER_TILED = 1, SCATTER_GENERIC = 2 };
uint64_t scatter_units_per_item(uint32_t mode, const ZgScatter &P, const uint64_t *max_sel_shape);

// Tiled scatter of uniform whole-chunk batches (k_scatter_tiled_p): per-plan constants of a batch
// whose every item is a whole chunk of full TILE x TILE tiles on 16-B aligned rows. Strides in
// elements; every offset inside a chunk and inside an item's output box fits 32 bits
// (tiled_persistent_params checks all of it).
struct ZgTiledP {
  uint32_t upi;                 // units per item (= scatter_units_per_item)
  uint32_t nta, ntl, nbg;       // tiles along A and Lx, slab groups along B
  uint32_t bext;                // extent of B (1: no B axis)
  uint32_t sL, sB, dA, dB;      // encoded stride of Lx and B, output stride of A and B
  uint32_t nrest;               // the other axes, innermost first: extent, encoded and output stride
  uint32_t rext[ZG_MAXD], rs[ZG_MAXD], rd[ZG_MAXD];
};
// false: the batch is not eligible (it keeps the one-unit-per-block kernel). geom: per item sel_start |
// sel_shape | out_start (3 * nd); origin[i] receives the output element offset of item i's origin.
bool tiled_persistent_params(const ZgScatter &P, const uint64_t *geom, size_t n_items, ZgTiledP &Q,
                             uint64_t *origin);
// whether n_items x upi units fit launch_scatter_tiled_p
bool tiled_persistent_fits(uint64_t n_items, uint64_t upi);

// Shard index: how launch_shard_index decodes every shard's index (bytes{endian} + optional crc32c chain).
struct ZgIndexSpec {
  uint64_t n_inner;      // inner chunks per shard
  uint64_t index_bytes;  // encoded index size (incl. checksums)
  uint32_t at_start;     // sharding index_location
  uint32_t big_endian;   // index bytes codec endianness
  uint32_t n_crc;        // number of crc32c codecs in the index chain (<= 4)
  uint32_t crc_at_start[4];
  uint32_t verify;       // validate_checksums
};

// blosc (c-blosc 1.x frames): a frame's compressor, as the decoder reads it from the header and the
// write path's layout (encode_layout.hpp) names it to the encoder
enum : uint32_t { BL_COMP_BLOSCLZ = 0, BL_COMP_LZ4 = 1, BL_COMP_SNAPPY = 2, BL_COMP_ZLIB = 3, BL_COMP_ZSTD = 4, BL_COMP_MEMCPY = 0x100,
                  BL_COMP_SKIP = 0xFFFFFFFFu };

}  // namespace zgpu

// device status codes (== zgpu.h)
#define ZG_OK 0u
#define ZG_INVALID_CHECKSUM 1u
#define ZG_DECODED_SIZE_MISMATCH 2u
#define ZG_SHARD_INDEX_OOB 3u
#define ZG_CORRUPT_STREAM 4u
#define ZG_INVALID_BYTE_RANGE 5u
#define ZG_UNSUPPORTED 6u
#define ZG_CRC_INPUT_TOO_SHORT 7u
#define ZG_SHARD_TOO_SMALL 8u
#define ZG_SHUFFLE_LENGTH 9u
