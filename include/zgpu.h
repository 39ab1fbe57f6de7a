/*
 * zgpu.h — C ABI of the MI355X-native Zarr chunk-decode codec pipeline (libzgpu.so).
 *
 * This is the drop-in boundary that a zarrs runtime codec plugin binds (see INTEGRATION.md for
 * the Rust FFI stub). Plain pointers and sizes only; no torch or HIP types in any signature.
 * Reference interfaces replaced (paths relative to the zarrs workspace root):
 *
 *   zgpu_chain_create   <- CodecChain::from_metadata + CodecChain::with_context
 *                          (zarrs/src/array/codec/array_to_bytes/codec_chain.rs:105-169,192-229),
 *                          Codec::from_metadata via the runtime registry
 *                          (zarrs_codec/src/lib.rs:279-318,372-449)
 *   zgpu_decode_batch   <- CodecChainBound::decode_into (codec_chain.rs:592-646) for full chunks and
 *                          ArrayPartialDecoderTraits::partial_decode_into
 *                          (zarrs_codec/src/codec_traits/array_partial_sync.rs:66-129) for partial
 *                          selections; for a sharding_indexed chain, ShardingCodecBound::decode_into
 *                          (sharding/sharding_codec.rs:617-707) and ShardingPartialDecoder
 *                          (sharding/sharding_partial_decoder_sync.rs:311-400). Batched: one call
 *                          decodes many chunks (per-chunk calls are a degenerate batch).
 *   zgpu_retrieve_array_subset
 *                       <- Array::retrieve_array_subset_into (zarrs/src/array/array_ops/
 *                          array_read_ops_common.rs:20-179, array_read_ops_array.rs:231-375):
 *                          the array-level batched driver that feeds zgpu_decode_batch.
 *   zgpu_retrieve_elements / zgpu_points_chunks
 *                       <- Indexer for &[ArrayIndices] / Vec<ArrayIndices> (zarrs_chunk_grid/src/indexer.rs:
 *                          285-392) read through ArrayPartialDecoderTraits::partial_decode(&dyn Indexer),
 *                          which partial_decode_fixed_indexer serves (sharding/
 *                          sharding_partial_decoder_sync.rs:492-560): elements by a list of coordinates.
 *   zgpu_decode_files / zgpu_retrieve_array_subset_files
 *                       <- the same, with the encoded chunks read from a filesystem store:
 *                          FilesystemStore::get / get_partial_many (zarrs_filesystem/src/lib.rs:
 *                          323-470) feeding array_read_ops_array.rs:290-300, with the reads of
 *                          one sub-batch overlapped with the H2D copy and decode of the previous.
 *   zgpu_encode_batch   <- CodecChain::encode (codec_chain.rs:528-555), fixed-size chains
 *   zgpu_encode_chunks  <- the same for variable-length chains: GzipCodec::encode (gzip_codec.rs:
 *                          96-107), ZstdCodec::encode (zstd_codec.rs:100-111), crc32c around them, and
 *                          ShardingCodecBound::encode_bounded (sharding_codec.rs:924-1085)
 *   zgpu_store_array_subset
 *                       <- Array::store_array_subset: store_chunk_with_options (zarrs/src/array/array_ops/
 *                          array_write_ops_array.rs:183-208), store_chunk_subset_with_options
 *                          (array_update_ops_array.rs:152-210) and, inside a shard, the inner-chunk
 *                          update of sharding/sharding_partial_encoder.rs
 *   zgpu_store_elements <- ArrayPartialEncoderTraits::partial_encode(&dyn Indexer, bytes) for a list of
 *                          coordinates: CodecPartialDefault (zarrs_codec/src/codec_partial_default.rs:
 *                          324-380) with update_array_bytes_indexer (zarrs_codec/src/array_bytes.rs:685-726)
 *   status codes        <- CodecError variants (zarrs_codec/src/lib.rs:617-686), 1:1 (see below).
 *
 * Threading: every entry point is thread-safe. Calls on one context run concurrently: each takes one
 * of the context's lanes (stream + copy streams; ZGPU_CTX_LANES, default 8) for its duration and
 * waits when all are busy; the context's pooled memory is shared under an allocator lock. A plan
 * serialises its own executes.
 * Stream ordering: a call runs on the caller's hip_stream (device inputs/outputs must be ready in
 * that stream's order), or with hip_stream NULL on the context's own stream, which first waits for
 * all work queued so far on the legacy default stream.
 * Memory: the caller owns every encoded input and the output; the library owns its scratch.
 */
#ifndef ZGPU_H
#define ZGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZGPU_MAX_DIMS 8

/* Status codes (per chunk and per call). Mapping onto zarrs_codec::CodecError:
 *  ZGPU_INVALID_CHECKSUM       -> CodecError::InvalidChecksum            (crc32c_codec.rs:130-133)
 *  ZGPU_DECODED_SIZE_MISMATCH  -> CodecError::UnexpectedChunkDecodedSize / InvalidBytesLength
 *                                 (ArrayBytes::validate, zarrs_codec/src/array_bytes.rs:376-386)
 *  ZGPU_SHARD_INDEX_OOB        -> CodecError::Other("The shard index references out-of-bounds
 *                                 bytes. The chunk may be corrupted.") (sharding_codec.rs:682-686)
 *  ZGPU_CORRUPT_STREAM         -> CodecError::IOError (gzip_codec.rs:116-118, zstd_codec.rs:119-128)
 *  ZGPU_INVALID_BYTE_RANGE     -> CodecError::InvalidByteRangeError
 *  ZGPU_UNSUPPORTED            -> CodecError::UnsupportedDataType / unsupported codec
 *  ZGPU_CRC_INPUT_TOO_SHORT    -> CodecError::Other("crc32c decoder expects a 32 bit input")
 *  ZGPU_SHARD_TOO_SMALL        -> CodecError::Other("The encoded shard is smaller than the
 *                                 expected size of its index.") (sharding_codec.rs:1277-1281)
 *  ZGPU_SHUFFLE_LENGTH         -> CodecError::Other("the shuffle codec expects the input byte
 *                                 length to be an integer multiple of the elementsize")
 *  ZGPU_INVALID_ARGUMENT       -> bad metadata / geometry (CodecCreateError, InvalidArraySubset)
 *  ZGPU_HIP_ERROR              -> device runtime failure (no zarrs equivalent)
 *  ZGPU_STORAGE_ERROR          -> StorageError::IOError from the filesystem store (open/read
 *                                 failures other than a missing key; zarrs_storage/src/lib.rs)
 *  ZGPU_CAST_NOT_REPRESENTABLE -> CodecError::Other from CastValueError::NotRepresentable ("scalar is
 *                                 not representable in target data type", zarrs_data_type/src/
 *                                 codec_traits/cast_value.rs): a cast_value chain met an element it
 *                                 cannot cast. Decode: the status of every descriptor whose SELECTION
 *                                 holds such an element (as zarrs' partial decoder, which casts only the
 *                                 selection); that descriptor's region of the output is unspecified,
 *                                 the call's other descriptors decode as usual, and a descriptor that
 *                                 already failed below the cast keeps that status. Encode and store:
 *                                 the entries have no per-chunk status, so the call fails, returns
 *                                 nothing, and zgpu_last_error names the first flat element index of
 *                                 the array (zarrs would fail only that chunk's store).
 */
enum {
  ZGPU_OK = 0,
  ZGPU_INVALID_CHECKSUM = 1,
  ZGPU_DECODED_SIZE_MISMATCH = 2,
  ZGPU_SHARD_INDEX_OOB = 3,
  ZGPU_CORRUPT_STREAM = 4,
  ZGPU_INVALID_BYTE_RANGE = 5,
  ZGPU_UNSUPPORTED = 6,
  ZGPU_CRC_INPUT_TOO_SHORT = 7,
  ZGPU_SHARD_TOO_SMALL = 8,
  ZGPU_SHUFFLE_LENGTH = 9,
  ZGPU_INVALID_ARGUMENT = 10,
  ZGPU_HIP_ERROR = 11,
  ZGPU_STORAGE_ERROR = 12,
  ZGPU_CAST_NOT_REPRESENTABLE = 13,
};

/* decode flags */
#define ZGPU_ENC_DEVICE 0x1u  /* desc.enc / chunk_ptrs are device pointers (else host memory)  */
#define ZGPU_OUT_DEVICE 0x2u  /* out is a device pointer (else host memory)                    */
#define ZGPU_NO_VALIDATE 0x4u /* override: CodecOptions::validate_checksums = false for the call */
#define ZGPU_DIRECT_IO 0x8u   /* filesystem reads: FilesystemStoreOptions::direct_io (O_DIRECT)   */
#define ZGPU_ONE_STREAM 0x10u /* every kernel of the call on hip_stream (no internal side stream,
                                 e.g. zstd's sequence decoder beside its literal decoder): for callers
                                 that run independent plans concurrently on streams of their own   */
#define ZGPU_ZSTD_LITS_FIRST 0x40u /* zstd, with ZGPU_ONE_STREAM: the plan decodes its Huffman literals
                                 before its sequences. For callers overlapping plans on streams of
                                 their own: a plan whose executor ends the overlap gets its literals
                                 (throughput-bound) done while the other plans decode sequences
                                 (latency-bound). Output identical either way.                     */

typedef struct zgpu_ctx zgpu_ctx;
typedef struct zgpu_chain zgpu_chain;
typedef struct zgpu_plan zgpu_plan;

/* One context per GPU: owns a HIP stream, device scratch and pinned staging. zgpu_ctx_destroy drops
 * the caller's reference: chains, plans and caches created on the context hold references of their
 * own, so the context is freed when the last of them is destroyed (any destruction order is safe). */
int zgpu_ctx_create(int hip_device, zgpu_ctx **out);
void zgpu_ctx_destroy(zgpu_ctx *ctx);
/* Live references of a context (1 + its chains, plans and caches; diagnostics and tests). */
int64_t zgpu_ctx_refcount(const zgpu_ctx *ctx);
/* Return the context's cached free device and pinned buffers to HIP (buffers in use stay). The
 * device pool also trims itself past ZGPU_POOL_CAP_MB (default 16 GiB) of free blocks. */
int zgpu_ctx_release_cached(zgpu_ctx *ctx);
/* The context's pooled memory in bytes (diagnostics and tests; any pointer may be NULL): device
 * blocks in use and cached free, pinned host blocks in use and cached free. */
int zgpu_ctx_pool_stats(const zgpu_ctx *ctx, uint64_t *dev_live, uint64_t *dev_free, uint64_t *host_live,
                        uint64_t *host_free);
/* Last error message of the calling thread on this context ("" if none). */
const char *zgpu_last_error(const zgpu_ctx *ctx);
const char *zgpu_status_name(int status);
/* Library version string, and the device kernels' ISA ("gfx950"). */
const char *zgpu_version(void);

/*
 * Parse and bind a codec chain.
 *  codecs_json : the Zarr V3 "codecs" JSON array (nested sharding_indexed configs included).
 *                Supported: transpose, bytes, sharding_indexed (nested to any depth, with codecs
 *                around the inner shardings and bytes->bytes codecs after any of them),
 *                crc32c (+numcodecs.crc32c), numcodecs.adler32 (location start, the default, or
 *                end), numcodecs.fletcher32, gzip, numcodecs.zlib, numcodecs.bz2 (decode only),
 *                zstd, numcodecs.shuffle, blosc (blosclz, lz4, lz4hc, zlib, snappy, zstd; shuffle /
 *                bitshuffle); the value codecs numcodecs.fixedscaleoffset, bitround and cast_value
 *                and (unsharded) packbits. Others -> ZGPU_UNSUPPORTED.
 *                cast_value ({"data_type", "rounding"?, "out_of_range"?, "scalar_map"?}, no other
 *                field) casts between any two of int8..int64, uint8..uint64, float16, bfloat16,
 *                float32, float64, bit-exact with zarrs: rounding nearest-even (default) /
 *                towards-zero / towards-positive / towards-negative / nearest-away, out_of_range
 *                absent / clamp / wrap (wrap with a float data_type: ZGPU_UNSUPPORTED), scalar_map
 *                {encode?, decode?} of up to 32 [key, value] pairs per direction (more:
 *                ZGPU_UNSUPPORTED), compared by the element's bits before the cast. Other data types
 *                (int2/4, uint2/4, float8 and the other micro-floats, bool, complex) and a
 *                configuration without data_type are ZGPU_UNSUPPORTED; a fill value that cannot be
 *                cast, or that does not decode back to itself, is ZGPU_INVALID_ARGUMENT. An element
 *                that cannot be cast: ZGPU_CAST_NOT_REPRESENTABLE (above).
 *                numcodecs.bz2 ({"level": 0..9}, required, no other field) reads the first bzip2
 *                stream of a chunk and ignores what follows it; the block CRCs and the combined
 *                CRC are checked whatever validate_checksums says, and a truncated, malformed or
 *                empty stream is ZGPU_CORRUPT_STREAM. Two deviations from libbz2: a block with the
 *                "randomised" bit (written by bzip2 0.9.0 and older only) is ZGPU_CORRUPT_STREAM,
 *                and a chunk whose stream holds more than 32 + slot bytes / 32768 block magics is
 *                ZGPU_DECODED_SIZE_MISMATCH with an unknown length, like any stream that outgrows
 *                its slot (libbz2 starts a new block every 99,981 symbols or more, so a stream
 *                of so many blocks that fits its chunk is hand-made). The stage's scratch is
 *                6.25 x the decoded bytes per chunk; ZGPU_BZ2_SCRATCH_MB (default 8192) bounds it,
 *                and a larger batch is decoded in rounds.
 *  data_type   : Zarr V3 data type name ("float32", "uint16", ...); fixed-size types only.
 *  fill        : native-endian fill value bytes (FillValue::as_ne_bytes), fill_len == dtype size.
 *  validate_checksums : CodecOptions::validate_checksums (zarrs default true, options.rs:24-33).
 */
int zgpu_chain_create(zgpu_ctx *ctx, const char *codecs_json, const char *data_type,
                      const void *fill, uint32_t fill_len, int validate_checksums,
                      zgpu_chain **out);
void zgpu_chain_destroy(zgpu_chain *chain);
/* Bytes per element of the bound data type. */
uint32_t zgpu_chain_element_size(const zgpu_chain *chain);

/* One chunk (or shard) to decode into the output array. */
typedef struct {
  const void *enc;                      /* encoded bytes; NULL = missing chunk -> fill value     */
  uint64_t enc_len;
  uint64_t chunk_shape[ZGPU_MAX_DIMS];  /* decoded chunk (shard) shape                          */
  uint64_t sel_start[ZGPU_MAX_DIMS];    /* wanted region of the chunk (chunk-relative)          */
  uint64_t sel_shape[ZGPU_MAX_DIMS];    /*   == chunk_shape & start 0 -> full decode path       */
  uint64_t out_start[ZGPU_MAX_DIMS];    /* where the region lands in the output array           */
} zgpu_chunk_desc;

/*
 * Decode n chunks into one C-order output array of shape out_shape[ndim].
 * A selection covering the whole chunk takes the full decode path (checksums verified);
 * a partial selection takes the partial-decoder path (crc32c stripped, not verified; for
 * sharding only the intersecting inner chunks are decoded), exactly as zarrs'
 * retrieve_chunk_subset_into does (array_read_ops_array.rs:346-375).
 * Output regions of different descriptors must be disjoint (ArrayBytesFixedDisjointView).
 * status[n] (optional) receives each chunk's status. Returns the first non-zero chunk status
 * (zarrs' try_for_each semantics) or a call-level error. hip_stream NULL = context stream.
 * A descriptor whose status is non-zero leaves its output region undefined (untouched, or partly
 * written: e.g. a blosc chunk decoded straight into the output, some of whose blocks failed), as
 * zarrs leaves a view whose decode_into failed; every other descriptor's region is complete.
 * The call is synchronous with respect to the host (statuses are final on return).
 * Any chain zgpu_chain_create accepts, and descriptors of different chunk shapes in one batch (e.g.
 * a rectilinear grid), decode here: one fused launch sequence per chunk shape when the chain is
 * "fused" (unsharded; or sharding_indexed, optionally behind transposes, with no bytes->bytes codec
 * after it and at most one plain nested sharding_indexed inside), else composed from fused ones:
 * whole-shard bytes->bytes codecs are decoded into device buffers first, and deeper or wrapped
 * nested shards are resolved through their outer index (read back) into descriptors of the inner
 * chain; transposes before a sharding_indexed of the second kind decode each selection in the
 * encoded (transposed) frame first, then transpose and scatter it.
 */
int zgpu_decode_batch(zgpu_chain *chain, uint32_t ndim, const zgpu_chunk_desc *descs,
                      uint64_t n, void *out, const uint64_t *out_shape, uint32_t flags,
                      int32_t *status, void *hip_stream);

/*
 * The output of a decode as a window of a larger C-order array: ArrayBytesDecodeIntoTarget /
 * ArrayBytesFixedDisjointView (zarrs_codec/src/array_bytes_fixed_disjoint_view.rs:12-207, the
 * target of CodecChainBound::decode_into, codec_chain.rs:592-646, and of
 * ShardingCodecBound::decode_into, sharding_codec.rs:617-707): base points at element [0,...,0] of
 * an array of array_shape; the view is the box [start, start + shape). Descriptors' out_start are
 * relative to the view (as with zgpu_decode_batch's out_shape = shape). Bytes of the array outside
 * the parts of the view the descriptors cover are never written.
 */
typedef struct {
  void *base;
  uint64_t array_shape[ZGPU_MAX_DIMS];
  uint64_t start[ZGPU_MAX_DIMS];
  uint64_t shape[ZGPU_MAX_DIMS];
} zgpu_out_view;

/* Concurrent-call coalescing (host inputs and host output only; ignored otherwise): calls carrying
 * this flag on the same chain, with the same flags and ndim, that arrive within the context's
 * collect window are decoded as ONE batch -- one packed H2D copy of their encoded bytes, one launch
 * sequence over all their chunks, one D2H copy -- and each caller gets its own statuses, its own
 * first-error return value and its own output window. This turns zarrs' per-shard decode_into calls
 * from rayon workers (array_read_ops_common.rs:173-176, sharding_codec.rs:617-707) into GPU-sized
 * batches without changing the read path. */
#define ZGPU_COALESCE 0x20u

/*
 * zgpu_decode_batch into a window of a larger array (host or device, ZGPU_OUT_DEVICE). A device
 * window is decoded in place (the scatter writes through the whole array's strides). A host window is
 * decoded into HBM and copied back box-wise (only the window's bytes cross PCIe; rows are placed by
 * host threads from pinned staging). Same statuses and return value as zgpu_decode_batch.
 */
int zgpu_decode_into(zgpu_chain *chain, uint32_t ndim, const zgpu_chunk_desc *descs, uint64_t n,
                     const zgpu_out_view *view, uint32_t flags, int32_t *status, void *hip_stream);

/*
 * zgpu_decode_batch with host inputs whose decoded output stays in library-owned pinned memory:
 * *data points at the C-order window of shape out_shape (prod(out_shape) * element size bytes),
 * valid until zgpu_result_release(*result). For callers that can only COPY into their target, as a
 * zarrs codec plugin must (ArrayBytesFixedDisjointView exposes copy_from_slice and no pointer,
 * zarrs_codec/src/array_bytes_fixed_disjoint_view.rs:177-206): decoding into a caller buffer and
 * then copying that into the view would cross host memory twice. ZGPU_COALESCE applies as for
 * zgpu_decode_batch (the pointer then lies inside the batch's pack, shared with its other callers).
 * On a failure *data is NULL and *result NULL. Host inputs only (ZGPU_ENC_DEVICE / ZGPU_OUT_DEVICE
 * -> ZGPU_INVALID_ARGUMENT).
 */
typedef struct zgpu_result zgpu_result;
int zgpu_decode_pinned(zgpu_chain *chain, uint32_t ndim, const zgpu_chunk_desc *descs, uint64_t n,
                       const uint64_t *out_shape, uint32_t flags, int32_t *status, const void **data,
                       zgpu_result **result);
void zgpu_result_release(zgpu_result *result);

/*
 * Coalescing policy of a context (ZGPU_COALESCE): a call waits at most window_us for other calls
 * to join its batch; a batch closes early at max_calls calls or max_bytes encoded bytes. Defaults:
 * 200 us, 8 calls, 1 GiB (env ZGPU_COALESCE_US / ZGPU_COALESCE_CALLS / ZGPU_COALESCE_BYTES).
 * Batches of one context run concurrently on its lanes.
 */
int zgpu_ctx_set_coalescing(zgpu_ctx *ctx, uint32_t window_us, uint32_t max_calls, uint64_t max_bytes);
/* Coalescing statistics of a context since its creation: batches executed and calls they carried. */
int zgpu_ctx_coalescing_stats(const zgpu_ctx *ctx, uint64_t *batches, uint64_t *calls);

/*
 * Prepared form of zgpu_decode_batch for device-resident inputs that are decoded repeatedly
 * (benchmarks, hipGraph capture): the descriptor table is planned and uploaded once. Plans take
 * fused chains and one chunk shape only (see zgpu_decode_batch); others -> ZGPU_UNSUPPORTED.
 * zgpu_plan_execute enqueues the decode on the stream and, if status != NULL, waits and returns
 * per-chunk statuses; with status == NULL it returns immediately after enqueue.
 * An asynchronous execute's output is valid only once zgpu_plan_status has returned for it: a blosc
 * input that outgrows the stream-table layout the plan recorded on its first execution is detected
 * on the device, nothing of it is decoded, and zgpu_plan_status re-runs the execution with a
 * read-back layout (ZGPU_CTR_BLOSC_RERUN) before it returns the statuses. Likewise a plan whose last
 * execution had no item for the serial zstd decoder skips that kernel; an input that needs it is
 * re-run by zgpu_plan_status with the kernel launched. A hipGraph capture of zgpu_plan_execute
 * therefore needs inputs whose blosc layout and zstd frame structure do not change between replays.
 */
int zgpu_plan_create(zgpu_chain *chain, uint32_t ndim, const zgpu_chunk_desc *descs, uint64_t n,
                     const uint64_t *out_shape, uint32_t flags, zgpu_plan **out);
int zgpu_plan_execute(zgpu_plan *plan, void *out, int32_t *status, void *hip_stream);
/* Wait for the plan's last execute on hip_stream and return its per-chunk statuses (first non-zero
 * status as the return value): lets independent plans (e.g. the levels of a multiscale pyramid)
 * run concurrently on separate streams. A status call is a call of its own for zgpu_last_counters and
 * zgpu_last_size_mismatch: after it they hold this plan's last execute alone, whichever other plan's
 * status the thread read before (zgpu_group_status likewise: the group's pieces summed once, the
 * failing descriptor in the group's status order). */
int zgpu_plan_status(zgpu_plan *plan, int32_t *status, void *hip_stream);
void zgpu_plan_destroy(zgpu_plan *plan);
/* Algorithmic HBM bytes of one execute (encoded bytes read + index bytes + decoded bytes
 * written), the figure bench.py prices the roofline with. */
uint64_t zgpu_plan_algorithmic_bytes(const zgpu_plan *plan);
/* The scatter kernel of the plan's last execute (before the first: the one the plan is eligible for).
 * Uniform batches of whole chunks of a transposing chain (full 64-wide tiles on 16-byte aligned
 * rows) take the tiled kernel that works from per-plan constants, ZGPU_SCATTER_TILED_PERSISTENT
 * (ZGPU_TILED_PERSIST=0 in the environment keeps the general tiled kernel; ZGPU_TILED_GRID=n makes n
 * workgroups loop over the batch instead of one workgroup per tile group). */
#define ZGPU_SCATTER_ROWS 0u
#define ZGPU_SCATTER_TILED 1u
#define ZGPU_SCATTER_GENERIC 2u
#define ZGPU_SCATTER_TILED_PERSISTENT 3u
uint32_t zgpu_plan_scatter_path(const zgpu_plan *plan);

/*
 * Plan group: one decode over the independent parts of a batch, each part one chunk shape and one
 * output (the levels of a multiscale pyramid; zarrs runs one rayon loop per array,
 * array_read_ops_common.rs:111-179). The group creates the parts' plans and places them on streams of
 * its own (at most ZGPU_GROUP_LANES, default 4 = HIP's default hardware queues): a part with at least
 * 1/(4 x lanes) of the group's encoded bytes gets a lane, the smaller parts share one lane (largest
 * first), the lanes left over go to the largest part, split into pieces of balanced encoded bytes; zstd
 * literals-first on the largest part's first piece and on the small-part lane (group.cpp). Part p has
 * n_descs[p] descriptors descs[p] decoded with chains[p] into an output of out_shapes[p] (ndim dims);
 * flags as zgpu_plan_create (ZGPU_ENC_DEVICE required). zgpu_group_execute enqueues every part behind
 * the work already on hip_stream (NULL: the legacy default stream) and makes hip_stream wait for all
 * of them; outs[p] is part p's output. status (NULL: asynchronous, read with zgpu_group_status)
 * receives the per-descriptor statuses, concatenated in part order; the return value is the first
 * non-zero one.
 */
typedef struct zgpu_group zgpu_group;
int zgpu_group_create(zgpu_chain *const *chains, uint32_t ndim, uint32_t n_parts, const zgpu_chunk_desc *const *descs,
                      const uint64_t *n_descs, const uint64_t *const *out_shapes, uint32_t flags, zgpu_group **out);
int zgpu_group_execute(zgpu_group *group, void *const *outs, int32_t *status, void *hip_stream);
int zgpu_group_status(zgpu_group *group, int32_t *status, void *hip_stream);
/* The group's plans: returns how many; for the first n, their lane, part and literals-first flag. */
uint32_t zgpu_group_layout(const zgpu_group *group, uint32_t *lane_of, uint32_t *part_of, uint32_t *lits_first,
                           uint32_t n);
uint64_t zgpu_group_algorithmic_bytes(const zgpu_group *group);
/* zgpu_plan_counters summed over the group's plans (after zgpu_group_status). */
uint32_t zgpu_group_counters(const zgpu_group *group, uint64_t *out, uint32_t n);
void zgpu_group_destroy(zgpu_group *group);

/* Device counters of a plan's last execute (after its statuses were read) or of the calling
 * thread's last decode call (zgpu_decode_batch / zgpu_decode_files / zgpu_retrieve_*), summed over
 * its sub-batches. Writes min(n, ZGPU_N_COUNTERS) values, returns how many were written. */
#define ZGPU_CTR_ENC_BYTES 0     /* encoded bytes read (resolved inner-chunk ranges of sharded items) */
#define ZGPU_CTR_ZSTD_SERIAL 1   /* zstd items decoded by the serial one-wave fallback decoder     */
#define ZGPU_CTR_ZSTD_PARALLEL 2 /* zstd items decoded by the block-parallel pipeline              */
#define ZGPU_CTR_BLOSC_RERUN 3   /* 1 when a blosc input outgrew the stream-table layout recorded by
                                    the plan's first execution and the execution was re-run with a
                                    read-back layout (later executions are asynchronous otherwise) */
#define ZGPU_CTR_BLOSC_BLOCKS 4  /* blosc blocks decoded: a partial selection decodes only the blocks
                                    covering the bytes it reads (blosc_partial_decoder.rs:33-60)     */
#define ZGPU_CTR_ITEMS 5         /* leaf items the call planned: chunks, or inner chunks of shards that meet
                                    the selection (each decoded, or filled when empty)                 */
#define ZGPU_CTR_ZSTD_LATENCY 6  /* zstd items finished by the window executor's latency mode (a subset
                                    of ZGPU_CTR_ZSTD_PARALLEL: small batches, one workgroup per window) */
#define ZGPU_CTR_BZ2_BLOCKS 7    /* bzip2 blocks decoded by the numcodecs.bz2 stage (each one is a unit of
                                    parallel work, whichever stream it came from)                      */
#define ZGPU_CTR_BZ2_ROUNDS 8    /* rounds the numcodecs.bz2 stage ran: 1 per execution whose scratch fits
                                    ZGPU_BZ2_SCRATCH_MB, more when the batch is cut; a whole-shard bz2
                                    stage adds the rounds of every run of its slot regrowing           */
#define ZGPU_CTR_STORE_DECODED 9 /* zgpu_store_array_subset: partly covered leaf chunks (chunks, or inner chunks
                                    of shards) whose old bytes were decoded for the read-modify-write    */
#define ZGPU_CTR_STORE_ENCODED 10 /* zgpu_store_array_subset: leaf chunks encoded                          */
#define ZGPU_CTR_STORE_CARRIED 11 /* zgpu_store_array_subset: untouched inner chunks whose encoded bytes were
                                    copied from the old shard into the new one                           */
#define ZGPU_CTR_POINT_LEAVES 12 /* zgpu_retrieve_elements: distinct leaves (chunks, or inner chunks of shards) the
                                    points touch: staged, read from the cache, or read as the fill value    */
#define ZGPU_CTR_POINT_ROUNDS 13 /* zgpu_retrieve_elements: decode + gather rounds: 1 when the touched leaves fit
                                    ZGPU_POINTS_SCRATCH_MB (and for the cache), more when they are cut     */
#define ZGPU_CTR_BLOSC_ALIASED 14 /* zstd blocks inside blosc frames that k_blosc_finish read where they lay
                                    (raw, RLE or literal-only blocks left out of the stream's slot: at most
                                    two per stream; 0 with ZGPU_BLOSC_ALIAS=0 and for serially decoded streams) */
#define ZGPU_N_COUNTERS 15
uint32_t zgpu_plan_counters(const zgpu_plan *plan, uint64_t *out, uint32_t n);
uint32_t zgpu_last_counters(uint64_t *out, uint32_t n);

/* Detail of the calling thread's last call that returned ZGPU_DECODED_SIZE_MISMATCH, for
 * CodecError::UnexpectedChunkDecodedSize(InvalidBytesLengthError::new(len, expected_len))
 * (zarrs_codec/src/lib.rs:491-501,632): the failing descriptor, the decoded length the final stage
 * saw and the expected length of the (inner) chunk. len == UINT64_MAX: a decompressor produced more
 * than expected_len bytes and stopped (its total is not known). Returns 1 if a detail is available. */
int zgpu_last_size_mismatch(uint64_t *desc, uint64_t *len, uint64_t *expected_len);

/*
 * Array::retrieve_array_subset_into over a regular chunk grid. chunk_ptrs/chunk_lens are
 * indexed by the C-order linear chunk-grid index (grid = ceil(array_shape/chunk_shape));
 * chunk_ptrs[i] == NULL means the key is missing (fill value). out holds prod(sel_shape)
 * elements in C order. Returns the first failing chunk's status.
 */
int zgpu_retrieve_array_subset(zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                               const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                               const uint64_t *chunk_lens, const uint64_t *sel_start,
                               const uint64_t *sel_shape, void *out, uint32_t flags,
                               void *hip_stream);

/*
 * Read by coordinates: Indexer for &[ArrayIndices] / Vec<ArrayIndices> (zarrs_chunk_grid/src/indexer.rs:
 * 285-392), served as partial_decode_fixed_indexer serves it (sharding/sharding_partial_decoder_sync.rs:
 * 492-560): every touched leaf is decoded once and the elements are picked out of it -- here in HBM.
 *
 * zgpu_points_chunks: the distinct C-order linear chunk-grid indices that the n points touch, ascending,
 * for a caller to look up only those keys in its store. Pure host code (no context, no device).
 * indices: [n][ndim] u64, row-major. *n_chunks receives their number; entries are written only while
 * they fit cap (call with cap 0 to size the array, as zgpu_store_classify). A coordinate >=
 * array_shape[d] (IndexerError::OutOfBounds): ZGPU_INVALID_ARGUMENT, and zgpu_last_error names the first
 * such point and its axis. n == 0: ZGPU_OK and no chunks.
 */
int zgpu_points_chunks(uint32_t ndim, const uint64_t *array_shape, const uint64_t *chunk_shape,
                       const uint64_t *indices, uint64_t n, uint64_t *chunks, uint64_t cap, uint64_t *n_chunks);
/*
 * The leaf grid zgpu_retrieve_elements works on, without a device: *n_leaves (optional) receives the
 * number of leaves of the array (chunk grid x leaves per chunk; leaf_shape NULL: the chunk is the leaf),
 * which the call holds against ZGPU_POINTS_BITMAP_MAX_BYTES * 8, and *wide (optional) whether its kernels
 * index with 64-bit arithmetic: 1 when an extent of the array or of the leaf, or the number of leaves,
 * does not fit 32 bits. ZGPU_INVALID_ARGUMENT for a zero extent, a chunk that is no multiple of the leaf,
 * or a grid of 2^64 leaves or more.
 */
int zgpu_points_geometry(uint32_t ndim, const uint64_t *array_shape, const uint64_t *chunk_shape,
                         const uint64_t *leaf_shape, uint64_t *n_leaves, uint32_t *wide);
/*
 * zgpu_retrieve_elements: out[i] = the element at indices[i] (out holds n elements: Indexer::output_shape
 * is [n]); duplicate points each get their element. chunk_ptrs / chunk_lens as for
 * zgpu_retrieve_array_subset (NULL: the key is missing, its points read the fill value); only the chunks
 * the points touch are read. flags: ZGPU_ENC_DEVICE, ZGPU_OUT_DEVICE and ZGPU_NO_VALIDATE as for decoding;
 * ZGPU_IDX_DEVICE: indices is device memory (host indices are uploaded; one path for both). Synchronous
 * with respect to the host, like zgpu_decode_batch. Every chain zgpu_decode_batch accepts works here.
 * The decode granule is the LEAF: the chunk, or, for a chain whose array->bytes codec is sharding_indexed,
 * the outermost sharding's inner chunk (carried back through the transposes in front of it into the
 * chunk's frame; value codecs in front of it change nothing about the rule). Each touched leaf whose key
 * is present is decoded once (ZGPU_CTR_ITEMS), in one batch per round, into staging bounded by
 * ZGPU_POINTS_SCRATCH_MB (environment, read per call; default 1024, a policy choice): more leaves than fit
 * take more rounds, at least one leaf each (ZGPU_CTR_POINT_ROUNDS). Checksums follow the descriptor rule of
 * zgpu_decode_batch: a whole unsharded chunk takes the full decode path and is verified; an inner chunk
 * of a shard takes the partial-decoder path: its crc32c is stripped, not verified, and the shard index
 * is verified.
 * Errors: a point out of bounds fails the whole call with ZGPU_INVALID_ARGUMENT before anything is decoded
 * or written (zgpu_last_error names the first such point); a kernel finds it, for host indices too. A
 * touched leaf that fails to decode gives the call that leaf's status, the first in ascending (chunk,
 * leaf) order; there is no per-point status: the elements taken from failed leaves are unspecified, all
 * others are complete. A corrupt leaf that no point touches does not matter. The touched leaves are found
 * through a dense bitmap of one bit per leaf of the array, limited to ZGPU_POINTS_BITMAP_MAX_BYTES
 * (16 MiB: 2^27 leaves); an array of more leaves returns ZGPU_UNSUPPORTED (no sparse fallback).
 * Element sizes 1, 2, 4, 8 and 16; a device out is aligned to min(element size, 8), indices to 8.
 */
#define ZGPU_IDX_DEVICE 0x100u
#define ZGPU_POINTS_BITMAP_MAX_BYTES (16u << 20)
int zgpu_retrieve_elements(zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                           const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                           const uint64_t *chunk_lens, const void *indices, uint64_t n,
                           void *out, uint32_t flags, void *hip_stream);

/*
 * zgpu_retrieve_array_subset over several GPUs of one node from one process (one chain per device,
 * each created on that device's context; same codecs and data type). The subset's chunk rows along
 * axis 0 are cut into n_dev contiguous groups and decoded concurrently, device d taking group d
 * (array_read_ops_common.rs:173-176: chunks are independent). Encoded chunks are host-resident
 * (ZGPU_ENC_DEVICE is rejected): each device uploads its own over its own link. Host `out`: every
 * device writes its rows straight into place. ZGPU_OUT_DEVICE: `out` is on chains[0]'s device; the
 * other devices decode into their own HBM and copy their rows into `out` peer-to-peer (xGMI).
 * Synchronous. Returns the first failing status in chunk (= device) order.
 */
int zgpu_retrieve_array_subset_multi(zgpu_chain *const *chains, uint32_t n_dev, uint32_t ndim,
                                     const uint64_t *array_shape, const uint64_t *chunk_shape,
                                     const void *const *chunk_ptrs, const uint64_t *chunk_lens,
                                     const uint64_t *sel_start, const uint64_t *sel_shape, void *out,
                                     uint32_t flags);

/*
 * Encoded chunks in a filesystem store. One byte range of one file per descriptor:
 * path = FilesystemStore::key_to_fspath(key) (zarrs_filesystem/src/lib.rs:173-179); path NULL or a
 * file that does not exist = missing key -> fill value (lib.rs:339-343,428-430); len == UINT64_MAX
 * reads from offset to the end of the file (ByteRange::FromStart(offset, None)); a range past the
 * end of the file gives that descriptor ZGPU_INVALID_BYTE_RANGE (lib.rs:437-447).
 */
typedef struct {
  const char *path;
  uint64_t offset;
  uint64_t len;
} zgpu_file_range;

/*
 * zgpu_decode_batch with descs[i].enc/enc_len taken from files[i] (the caller's enc fields are
 * ignored). The batch is cut into sub-batches (in descriptor order); a pool of host threads reads
 * sub-batch k+1 with positional reads (O_DIRECT page reads with ZGPU_DIRECT_IO, falling back to
 * buffered reads where the filesystem has no O_DIRECT) into pinned staging while sub-batch k is
 * copied to HBM and decoded. out is device memory (ZGPU_OUT_DEVICE) or host memory.
 * Hard I/O errors (not ENOENT) fail the call with ZGPU_STORAGE_ERROR.
 */
int zgpu_decode_files(zgpu_chain *chain, uint32_t ndim, const zgpu_chunk_desc *descs,
                      const zgpu_file_range *files, uint64_t n, void *out, const uint64_t *out_shape,
                      uint32_t flags, int32_t *status, void *hip_stream);

/*
 * zgpu_retrieve_array_subset over a filesystem store: chunk_paths[i] is the path of the chunk with
 * C-order linear grid index i (NULL or nonexistent = missing key); each chunk file is read whole.
 */
int zgpu_retrieve_array_subset_files(zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                                     const uint64_t *chunk_shape, const char *const *chunk_paths,
                                     const uint64_t *sel_start, const uint64_t *sel_shape, void *out,
                                     uint32_t flags, void *hip_stream);

/*
 * Write path: CodecChain::encode (zarrs/src/array/codec/array_to_bytes/
 * codec_chain.rs:528-555) for fixed-size chains -- transpose, bytes (endianness), numcodecs.shuffle
 * (innermost, elementsize = data type size), crc32c / numcodecs.adler32 (end or start) and
 * numcodecs.fletcher32, any number of them. Compressing codecs
 * and sharding_indexed return ZGPU_UNSUPPORTED here: they go through zgpu_encode_chunks.
 * zgpu_chain_encoded_size: encoded bytes of one chunk of chunk_shape (BytesRepresentation::FixedSize),
 * -1 if the chain's encoded size is not fixed.
 * zgpu_encode_batch: encode the chunks whose origins are descs[i].chunk_start (in elements) of the
 * device-resident C-order array (array_shape) into descs[i].dst (device memory, >= encoded size).
 * Chunk regions past the array edge encode the fill value. flags must be
 * ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE.
 */
typedef struct {
  void *dst;
  uint64_t dst_cap;
  uint64_t chunk_start[ZGPU_MAX_DIMS];
} zgpu_encode_desc;
int64_t zgpu_chain_encoded_size(const zgpu_chain *chain, uint32_t ndim, const uint64_t *chunk_shape);
int zgpu_encode_batch(zgpu_chain *chain, uint32_t ndim, const uint64_t *chunk_shape, const void *array,
                      const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint32_t flags,
                      void *hip_stream);
/*
 * zgpu_encode_batch plus the variable-length chains: gzip (one DEFLATE stream of dynamic-Huffman or
 * stored blocks in a gzip member, k_gzip_encode), zstd (one single-segment frame of 64 KiB blocks:
 * Huffman / RLE / raw literals, predefined-FSE sequences, optional XXH64 content checksum; encoded in
 * 1 MiB segments, one wave each, k_zstd_encode_seg + k_zstd_frame), numcodecs.zlib (the same DEFLATE
 * stream in an RFC 1950 wrapper with its Adler-32 trailer), crc32c / adler32 / fletcher32 around them,
 * the fixed-size stages in front, and sharding_indexed over a fixed-size or compressing inner chain
 * (ShardingCodecBound::encode_bounded, sharding_codec.rs:924-1085, with SubchunkWriteOrder::C: inner
 * chunks in C order of the inner grid, an inner chunk equal to the fill value everywhere omitted,
 * index bytes{endian} + crc32c at the start or end). The compressed bytes are valid streams that
 * every gzip / zlib / zstd decoder reads back to the input; they are not byte-identical to zlib's,
 * flate2's or libzstd's output (the Zarr specification fixes the decoded bytes, not the encoder). blosc
 * (BloscCodec::encode, blosc_codec_via_blosc_src.rs:113-128) writes c-blosc 1.x frames with
 * blosclz, lz4 / lz4hc, snappy, zlib or zstd streams after a byte shuffle / bitshuffle (frames any
 * c-blosc 1.x decoder reads, not byte-identical to c-blosc's).
 * enc_lens[n] receives each chunk's encoded length; descs[i].dst_cap must be >=
 * zgpu_chain_encoded_bound. numcodecs.bz2 has no encoder on the GPU: a chain with it returns
 * ZGPU_UNSUPPORTED here, while zgpu_chain_encoded_bound still gives Bz2Codec's bound for it
 * (bz2_codec.rs: size + size / 8 + 1024). zgpu_chain_encoded_bound: the fixed size, or the worst case
 * (gzip_codec.rs:122-136, zlib_codec.rs encoded_representation, zstd_codec.rs:132-147; a shard: every inner chunk at its bound + index),
 * -1 if unbounded.
 */
int64_t zgpu_chain_encoded_bound(const zgpu_chain *chain, uint32_t ndim, const uint64_t *chunk_shape);
/* One chunk (or shard) of chunk_shape from host bytes (C order), encoded on the GPU as
 * zgpu_encode_chunks does; *enc / *enc_len: the encoded bytes in library-owned pinned memory, valid
 * until zgpu_result_release(*result) -- the codec plugin's CodecChain::encode /
 * ShardingCodecBound::encode (sharding_codec.rs:351-376), which must return owned host bytes. */
int zgpu_encode_pinned(zgpu_chain *chain, uint32_t ndim, const uint64_t *chunk_shape, const void *decoded,
                       const void **enc, uint64_t *enc_len, zgpu_result **result);
int zgpu_encode_chunks(zgpu_chain *chain, uint32_t ndim, const uint64_t *chunk_shape, const void *array,
                       const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint32_t flags,
                       uint64_t *enc_lens, void *hip_stream);

/*
 * Array::store_array_subset over a regular chunk grid (zarrs/src/array/array_ops/
 * array_write_ops_array.rs:183-208, store_chunk_with_options; array_update_ops_array.rs:152-210,
 * store_chunk_subset_with_options; for sharded arrays the inner-chunk update of
 * sharding/sharding_partial_encoder.rs). The subset [sel_start, sel_start + sel_shape) of the array takes
 * the values of `data` (C order, native-endian elements). The unit of read-modify-write is the leaf
 * chunk: the chunk, or for a sharding_indexed chain (one level, nothing around it, index = bytes +
 * crc32c codecs) the inner chunk. For every leaf chunk of every chunk the subset meets:
 *   covered (its whole box lies inside the subset): encoded from `data`; the old bytes are not read;
 *   partly covered: the old leaf chunk is decoded in full (checksums verified; missing = fill value),
 *     the overlap pasted in (k_subset_overlay) and the result encoded; elements past the array's edge
 *     keep what the old chunk decoded to;
 *   untouched (inner chunks only): neither decoded nor encoded; its encoded bytes are copied from the
 *     old shard as its index gives them (not checksum-verified), an absent one stays absent.
 * A leaf chunk whose new content equals the fill value bytewise in every element is not written
 * (store_empty_chunks = false, array_write_ops_array.rs:192-199): the chunk is erased, the inner chunk
 * omitted from its shard. ZGPU_STORE_EMPTY_CHUNKS stores such chunks (inner chunks are omitted all the
 * same, as the sharding codec omits them). A shard left without an inner chunk is erased. New shards
 * are laid out as zgpu_encode_chunks lays them out.
 * chunk_ptrs / chunk_lens: the old encoded chunks as for zgpu_retrieve_array_subset; only chunks that
 * the subset meets without covering are read (zgpu_store_classify tells which).
 * flags: ZGPU_ENC_DEVICE: the old chunks are device memory and every entry's enc is device memory;
 * otherwise host memory in, pooled pinned host memory out. ZGPU_OUT_DEVICE: `data` is device memory.
 * ZGPU_NO_VALIDATE as for decoding. *entries: one entry per chunk the subset meets, in C order of the
 * chunk grid, valid with their enc until zgpu_result_release(*result). An entry whose old bytes failed
 * to decode (or whose old shard index is corrupt: ZGPU_INVALID_CHECKSUM, or points outside the shard:
 * ZGPU_SHARD_INDEX_OOB, checked for every entry, those of untouched inner chunks included) carries that
 * status and no action; the other entries are valid. Returns the first non-zero entry status, or a
 * call-level error (*entries NULL): ZGPU_UNSUPPORTED, before any GPU work, for a chain
 * zgpu_encode_chunks refuses, for codecs around sharding_indexed, nested sharding, or value codecs or
 * packbits with sharding; ZGPU_INVALID_ARGUMENT for a subset outside the array. A zero-volume subset is
 * ZGPU_OK with no entries and no result. Synchronous on hip_stream. No locking (zarrs' is commented
 * out): the caller serialises writers of one chunk.
 */
#define ZGPU_STORE_EMPTY_CHUNKS 0x80u
#define ZGPU_STORE_SET 1
#define ZGPU_STORE_ERASE 2
typedef struct {
  uint64_t chunk;   /* C-order linear chunk-grid index */
  uint32_t action;  /* ZGPU_STORE_SET / ZGPU_STORE_ERASE; 0 when status != 0 */
  int32_t status;
  const void *enc;  /* ZGPU_STORE_SET: the chunk's new encoded bytes */
  uint64_t enc_len;
} zgpu_store_entry;
int zgpu_store_array_subset(zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                            const uint64_t *chunk_shape, const void *const *chunk_ptrs, const uint64_t *chunk_lens,
                            const uint64_t *sel_start, const uint64_t *sel_shape, const void *data, uint32_t flags,
                            const zgpu_store_entry **entries, uint64_t *n_entries, zgpu_result **result,
                            void *hip_stream);
/* One ZGPU_STORE_SET entry's encoded bytes copied to dst (enc_len bytes; host or device memory,
 * whichever side enc is on) before the result is released: for stores that keep buffers of their own.
 * Synchronous on hip_stream. */
int zgpu_store_entry_copy(zgpu_chain *chain, const zgpu_store_entry *entry, void *dst, void *hip_stream);
/*
 * The store by coordinates: ArrayPartialEncoderTraits::partial_encode(indexer, bytes) for a list of
 * ArrayIndices. data[i] (n native-endian elements) becomes the element at indices[i] ([n][ndim] uint64,
 * row-major, 8-byte aligned). A coordinate that appears more than once takes the value of the point with
 * the HIGHEST i: for an unsharded chunk zarrs serves the call by CodecPartialDefault (zarrs_codec/src/
 * codec_partial_default.rs:324-380: decode, update_array_bytes, encode), and update_array_bytes_indexer
 * (zarrs_codec/src/array_bytes.rs:685-726) copies the update elements in indexer order, so the last one
 * stays; the result here is exactly that. For sharding_indexed the reference has no such path yet
 * (sharding/sharding_partial_encoder.rs:196-201, "does not yet support partial encoding with generic
 * indexers"); the result here is what zarrs gives when the points are stored one after another, in
 * order, as one-element subsets through its box path, i.e. the inner-chunk update zgpu_store_array_subset
 * implements.
 * Chains: exactly those zgpu_store_array_subset accepts, with the same refusals (ZGPU_UNSUPPORTED before
 * any GPU work); the granule is the same leaf chunk. EVERY touched leaf is treated as partly covered:
 * its old bytes are decoded in full, once, all touched leaves in one batch (checksums as for
 * zgpu_store_array_subset; a missing key or an absent inner chunk reads as the fill value), the points
 * are scattered into the decoded leaves in HBM (k_points_claim: per element the highest i;
 * k_points_scatter: the winners write), and from there everything is zgpu_store_array_subset's: the fill
 * check, the encode of what is not all fill, the shard layout with untouched inner chunks carried byte
 * for byte, the erasure of a leaf or shard left all fill or empty, ZGPU_STORE_EMPTY_CHUNKS.
 * chunk_ptrs / chunk_lens: as for zgpu_retrieve_elements; only the chunks the points touch are read
 * (zgpu_points_chunks tells which). *entries: one entry per chunk that holds a touched leaf, in C order of
 * the chunk grid; a failing chunk carries its status and no action (its points are dropped), the others
 * are valid; the call returns the first non-zero status. Lifetimes as for zgpu_store_array_subset.
 * flags: ZGPU_ENC_DEVICE: old chunks and entries' enc are device memory; ZGPU_OUT_DEVICE: `data` is
 * device memory, aligned to min(element size, 8); ZGPU_IDX_DEVICE: indices is device memory;
 * ZGPU_NO_VALIDATE, ZGPU_STORE_EMPTY_CHUNKS. One path: host indices and data are uploaded first.
 * A point out of bounds fails the whole call with ZGPU_INVALID_ARGUMENT before anything is decoded (found
 * by k_points_mark; the message names the smallest such point and its axis; *entries NULL). There is no
 * per-point status. n == 0: ZGPU_OK, no entries, no result. Element sizes 1, 2, 4, 8 and 16. Limits,
 * ZGPU_UNSUPPORTED with a message that says so, before any device work: the bitmap of one bit per leaf
 * (ZGPU_POINTS_BITMAP_MAX_BYTES, as for the read), and n >= 2^32 - 1 (the winner table holds i + 1 in 32
 * bits). All touched leaves are staged at once (no rounds, unlike the read): decoded leaf bytes plus 4
 * bytes of winner table per staged element; when that allocation fails the message gives both figures.
 * Counters: ZGPU_CTR_POINT_LEAVES, ZGPU_CTR_STORE_DECODED / _ENCODED / _CARRIED. Synchronous on
 * hip_stream. No locking, and no cache is invalidated.
 */
int zgpu_store_elements(zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                        const uint64_t *chunk_shape, const void *const *chunk_ptrs, const uint64_t *chunk_lens,
                        const void *indices, uint64_t n, const void *data, uint32_t flags,
                        const zgpu_store_entry **entries, uint64_t *n_entries, zgpu_result **result,
                        void *hip_stream);
/*
 * The host's classification behind zgpu_store_array_subset, without a device: the chunks the subset
 * meets in C order of the chunk grid (chunks[k]: linear index) and, per chunk, the class of each of its
 * leaf chunks in C order of the inner grid (leaf_class[k * leaves_per_chunk + j]; leaf_shape NULL or
 * equal to chunk_shape: one leaf per chunk). *n_chunks receives the number of chunks met; entries are
 * written only while they fit cap (call with cap 0 to size the arrays). A chunk must be fetched from
 * the store unless every leaf of it is ZGPU_LEAF_COVERED.
 */
#define ZGPU_LEAF_UNTOUCHED 0
#define ZGPU_LEAF_PARTIAL 1
#define ZGPU_LEAF_COVERED 2
int zgpu_store_classify(uint32_t ndim, const uint64_t *array_shape, const uint64_t *chunk_shape,
                        const uint64_t *leaf_shape, const uint64_t *sel_start, const uint64_t *sel_shape,
                        uint64_t *chunks, uint8_t *leaf_class, uint64_t cap, uint64_t *n_chunks);

/*
 * HBM-resident decoded-chunk cache: ChunkCacheDecodedLruSizeLimit (zarrs/src/array/chunk_cache/
 * chunk_cache_lru.rs:270) used through ArrayCached::retrieve_array_subset (zarrs/src/array/array_ops/
 * array_read_ops_array_cached.rs:315-412). One cache per array (as an ArrayCached owns its cache):
 * whole decoded chunks (full decode path, checksums verified) in a pool of floor(capacity / chunk
 * bytes) HBM slots, keyed by the C-order chunk-grid index; a missing key is cached as "no chunk" (fill
 * value); least recently used chunks are evicted. A read decodes all of its misses into their slots in
 * one batch, then gathers the subset from HBM. A read touching more chunks than the cache holds is
 * decoded directly (nothing new cached). Arguments as zgpu_retrieve_array_subset.
 */
typedef struct zgpu_cache zgpu_cache;
int zgpu_cache_create(zgpu_ctx *ctx, uint64_t capacity_bytes, zgpu_cache **out);
void zgpu_cache_destroy(zgpu_cache *cache);
int zgpu_cache_clear(zgpu_cache *cache);
int zgpu_cache_stats(zgpu_cache *cache, uint64_t *hits, uint64_t *misses, uint64_t *entries, uint64_t *bytes_used);
int zgpu_cache_retrieve_array_subset(zgpu_cache *cache, zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                                     const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                                     const uint64_t *chunk_lens, const uint64_t *sel_start, const uint64_t *sel_shape,
                                     void *out, uint32_t flags, void *hip_stream);

/*
 * zgpu_retrieve_elements through the cache (ArrayCached with an Indexer of coordinates). The granule is the
 * chunk, which is what the cache holds: the touched chunks that miss are decoded whole into their slots in
 * one batch (verified, as a subset read), the elements are then gathered straight from the pool (no
 * staging, one round). Hits and misses count each touched chunk once. A read touching more chunks than
 * the cache holds takes zgpu_retrieve_elements' path and caches nothing new.
 */
int zgpu_cache_retrieve_elements(zgpu_cache *cache, zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                                 const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                                 const uint64_t *chunk_lens, const void *indices, uint64_t n, void *out,
                                 uint32_t flags, void *hip_stream);

/*
 * DLPack export of a decoded subset left in HBM (the reference exports CPU tensors only:
 * zarrs/src/array/array_dlpack_ext.rs:44-70, Device::CPU). The zgpu_dl_* types are layout-identical to
 * DLPack's DLDevice / DLDataType / DLTensor / DLManagedTensor (dlpack.h, unversioned ABI, consumed
 * through a PyCapsule named "dltensor"); device_type is kDLROCM (10). The library allocates the buffer
 * on the chain's device; the consumer calls deleter(tensor) when done. cache may be NULL.
 */
#define ZGPU_DL_ROCM 10
typedef struct { int32_t device_type; int32_t device_id; } zgpu_dl_device;
typedef struct { uint8_t code; uint8_t bits; uint16_t lanes; } zgpu_dl_data_type;
typedef struct {
  void *data;
  zgpu_dl_device device;
  int32_t ndim;
  zgpu_dl_data_type dtype;
  int64_t *shape;
  int64_t *strides; /* NULL: compact row-major */
  uint64_t byte_offset;
} zgpu_dl_tensor;
typedef struct zgpu_dl_managed_tensor {
  zgpu_dl_tensor dl_tensor;
  void *manager_ctx;
  void (*deleter)(struct zgpu_dl_managed_tensor *self);
} zgpu_dl_managed_tensor;
int zgpu_retrieve_array_subset_dlpack(zgpu_cache *cache, zgpu_chain *chain, uint32_t ndim, const uint64_t *array_shape,
                                      const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                                      const uint64_t *chunk_lens, const uint64_t *sel_start, const uint64_t *sel_shape,
                                      uint32_t flags, void *hip_stream, zgpu_dl_managed_tensor **out);

#ifdef __cplusplus
}
#endif
#endif /* ZGPU_H */
