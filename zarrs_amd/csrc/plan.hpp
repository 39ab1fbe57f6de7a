// The fused decode plan on the device and what the host translation units of libzgpu share around it:
// the chain handle, the plan's entry points (plan_exec.cpp), the composed decode (general.cpp) and the
// result object. A plan is one PlanLayout -- everything the host decided about the batch, a plain value
// made without the device (plan_layout.hpp) and constant for the plan's life -- plus the device state
// built from it: buffers, streams, and what its executions found out (capacities, counters, the path
// the last scatter took).
#pragma once
#include <memory>
#include <mutex>
#include <vector>

#include "chain.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "encode_layout.hpp"
#include "kernels/launch.hpp"
#include "plan_layout.hpp"

using namespace zgpu;  // (a private header: only libzgpu's own translation units include it)

#pragma GCC visibility push(hidden)
struct zgpu_chain {
  zgpu_ctx *ctx;
  std::shared_ptr<Chain> chain;
  bool validate;
};

// ------------------------------------------------------------------------------------------------
// Plan
// ------------------------------------------------------------------------------------------------
// A stream beside the one a plan runs on, with the two events that order work between them; created on
// first use with the priority of the stream it first runs beside.
struct SideLane {
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  void ensure(hipStream_t like) {
    if (stream) return;
    int prio = 0;
    if (like) (void)hipStreamGetPriority(like, &prio);
    HIPCHK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio));
    for (hipEvent_t &e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  void destroy() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct zgpu_plan {
  zgpu_ctx *ctx;   // holds a reference (dropped by the destructor)
  PoolBlocks mem;  // every device and pinned buffer below, for the plan's lifetime
  const PlanLayout L;  // the host's decisions (leaf points into `chain`, or is null)
  zgpu_plan(zgpu_ctx *c, PlanLayout &&layout) : ctx(c), mem(c), L(std::move(layout)), last_path(L.first_path) {
    ctx_ref(c);
  }
  std::mutex mu;  // one execute / status at a time per plan
  Lane own{};     // the plan's stream for executes without a caller stream (lazy)
  std::shared_ptr<Chain> chain;
  bool validate = true;
  uint32_t nd = 0;
  uint64_t n_desc = 0;
  uint32_t flags = 0;
  std::vector<uint64_t> out_shape;
  // the layout's tables on the device
  ZgItem *d_items = nullptr, *d_items_init = nullptr;
  uint64_t *d_geom = nullptr;
  uint32_t *d_status = nullptr;
  ZgShard *d_shards = nullptr;
  uint64_t *d_index = nullptr;
  uint32_t *d_shard_status = nullptr;
  // nested sharding: middle shard records (resolved through the outer index each execution), their
  // status, the middle shards as a shard table, and their decoded indexes
  ZgItem *d_mids = nullptr, *d_mids_init = nullptr;
  uint32_t *d_mid_status = nullptr, *d_shard_status2 = nullptr;
  ZgShard *d_mid_shards = nullptr;
  uint64_t *d_index2 = nullptr;
  uint8_t *d_pool[2] = {nullptr, nullptr};
  uint64_t *d_origin = nullptr;  // tiled_p: L.origin
  unsigned long long *d_counter = nullptr;
  // control block: [counter (256 B) | per-item status (4 B each)], cleared by ONE memset and read
  // back by ONE D2H copy into pinned memory (h_ctl) per execute
  uint8_t *d_ctl = nullptr, *h_ctl = nullptr;
  size_t ctl_bytes = 0;
  uint64_t in_len_hint = 0;  // the longest item before any stage, as far as the host knows: how many
                             // workgroups a checksum stage gives an item (k_linsum_strip), not its result
  // scratch grown on demand
  struct Grow {
    void *p = nullptr;
    size_t n = 0;
  };
  void *grow(Grow &g, size_t bytes) {
    if (g.n < bytes) {
      g.p = mem.regrow(g.p, bytes);
      g.n = bytes;
    }
    return g.p;
  }
  Grow ck_parts;   // the adler32 / fletcher32 stages' range sums
  Grow live_list;  // the rows scatter's list of items still to write (ZGPU_SCATTER_LIST)

  struct {
    ZstdScratch zs{};  // block-parallel zstd scratch (allocated when the chain has zstd)
    SideLane side;     // side stream of the zstd sequence decoder (ZGPU_ONE_STREAM keeps one stream)
    // serial fallback: skipped once an execution of this plan had no serial item (a later one that
    // has some is re-run by plan_statuses with the fallback launched)
    bool serial_off = false, serial_skipped = false;
  } zstd;
  void zstd_fork(ZstdScratch &Z, hipStream_t s) {
    if (flags & ZGPU_ONE_STREAM) return;
    zstd.side.ensure(s);
    Z.side = zstd.side.stream;
    Z.ev_fork = zstd.side.ev[0];
    Z.ev_join = zstd.side.ev[1];
  }
  // blosc stage scratch (the stream table is sized from the frame headers)
  struct {
    Grow info, bases, subs, sub_status, sub_kind, blocks, tmp, zaux, lzl, zseg;
    Grow zs[ZSTD_SCRATCH_BUFFERS];  // the zstd streams' scratch (zstd_bind)
    BlCaps caps{};  // stream-table capacities recorded by the first execution
    bool caps_valid = false, caps_seen = false;
    uint8_t *h = nullptr;        // pinned: BlInfo read-back (first execution)
    uint64_t *d_need = nullptr;  // L.bl_need
  } blosc;
  struct {
    uint32_t *d_order = nullptr;  // LPT dispatch order of the items
    uint32_t *d_seg = nullptr;    // symbol-record scratch of the segmented decode
    Grow crc;                     // ZGPU_GZIP_CRC_FORK: snapshots for the trailing crc32c's side check
  } gzip;
  struct {
    Bz2Scratch bz{};      // block records, BWT vectors and pre-RLE1 bytes of one round of items
    uint64_t rounds = 0;  // rounds the last enqueue launched (ZGPU_CTR_BZ2_ROUNDS)
  } bz2;
  // what the executions left behind
  uint32_t last_path;  // zgpu_plan_scatter_path: of the last enqueue (before one: the layout's)
  uint64_t last_enc_bytes = 0;
  uint64_t last_counters[CTR_N] = {};
  uint8_t *last_out = nullptr;  // output of the last enqueue (a blosc layout overflow re-runs into it)

  ~zgpu_plan() {
    struct Unref {
      zgpu_ctx *c;
      ~Unref() { ctx_unref(c); }
    } unref{ctx};  // after every buffer went back to the context's pools
    if (own.stream) {
      (void)hipStreamSynchronize(own.stream);
      (void)hipStreamDestroy(own.stream);
    }
    if (own.order_ev) (void)hipEventDestroy(own.order_ev);
    zstd.side.destroy();
    mem.release();
  }
};

// plan_exec.cpp
zgpu_plan *plan_new(zgpu_ctx *ctx, const std::shared_ptr<Chain> &chain, bool validate, uint32_t nd,
                    const zgpu_chunk_desc *descs, uint64_t n, const uint64_t *out_shape, uint32_t flags);
void plan_upload(zgpu_plan &P, hipStream_t us);
void plan_enqueue(zgpu_plan &P, uint8_t *out, hipStream_t s);
int plan_statuses(zgpu_plan &P, int32_t *status, hipStream_t s);
hipStream_t pick_stream(Lane *L, void *s);
Lane *plan_lane(zgpu_plan &P);
// zgpu.cpp
uint64_t volume(const uint64_t *shape, uint32_t nd);

struct CoBatch;
// zgpu_decode_pinned's result: a pooled pinned buffer of the context, or a slice of a coalesced
// batch's pack (the batch, and with it the pack, lives until every caller released its result)
struct zgpu_result {
  zgpu_ctx *ctx = nullptr;
  uint8_t *own = nullptr;             // pooled pinned buffer (uncoalesced call)
  std::shared_ptr<CoBatch> batch;     // coalesced call: the batch holding the pack
  uint8_t *dev = nullptr;             // pooled device buffer (zgpu_store_array_subset with ZGPU_ENC_DEVICE)
  std::vector<zgpu_store_entry> store_entries;  // zgpu_store_array_subset's entries (enc inside own / dev)
  ~zgpu_result() {
    if (own) ctx->host_free(own);
    if (dev) ctx->dev_free(dev);
    batch.reset();
    ctx_unref(ctx);
  }
};

// general.cpp
struct GeneralCall {
  zgpu_ctx *C;
  bool validate;
  uint32_t nd;
  uint8_t *out;  // device output array
  const uint64_t *out_shape;
  uint32_t flags;
  hipStream_t s;
  std::vector<std::unique_ptr<zgpu_plan>> keep;  // whole-shard decode slots, alive until the call ends
};
void decode_general(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs, uint64_t n,
                    int32_t *status);
bool fused_plannable(const Chain &top);
bool uniform_shapes(const zgpu_chunk_desc *descs, uint64_t n, uint32_t nd);
bool desc_geometry_ok(const zgpu_chunk_desc &D, uint32_t nd, const uint64_t *out_shape);
uint64_t sel_volume(const zgpu_chunk_desc &D, uint32_t nd);
std::shared_ptr<Chain> strip_value_codecs(const Chain &c, std::vector<Codec> &steps);
void retype_stripped(Chain &c, const Chain &original);
uint8_t *value_encode_elements(const std::vector<Codec> &steps, const uint8_t *in, uint64_t n, Scratch &sc,
                               hipStream_t s, uint64_t *fail);
// write.cpp: zgpu_encode_chunks (arguments checked) on stream s, synchronous; fixed_only: refuse a chain
// whose chunks vary in length (zgpu_encode_batch)
int encode_chunks_on(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                     const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                     hipStream_t s, bool fixed_only = false);
// The checksum codecs of an ENC_FIXED layout in place over n device buffers (d_dst on the device): each
// covers [lo, lo + in_bound) of every buffer and writes its value in front of or behind them.
void checksums_in_place(const uint64_t *d_dst, uint32_t n, const EncodeLayout &L, hipStream_t s);
// The device tables that lay out n shards of n_chunks inner chunks in all and the launch's arguments from
// the sharded layout L: dst = h_dst (copied on s); the launch fills off, index_ptr and len; nf: nf_words
// words, the fill flags first. Then checksums_in_place(index_ptr, n, *L.index, s) finishes the shards.
struct ShardTables {
  uint64_t *dst, *index_ptr, *len, *off;
  uint32_t *nf;
  ZgShardLayoutArgs A;
};
ShardTables shard_tables(Scratch &sc, const EncodeLayout &L, const uint64_t *h_dst, uint64_t n, uint64_t n_chunks,
                         uint64_t nf_words, uint64_t E, uint64_t E_pitch, hipStream_t s);
#pragma GCC visibility pop
