// The fused decode plan and what the host translation units of libzgpu share around it: the chain
// handle, the plan's entry points (zgpu.cpp), the composed decode (general.cpp) and the result object.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

#include "chain.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "kernels/launch.hpp"

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
enum StageKind { ST_CRC32C, ST_GZIP, ST_ZSTD, ST_UNSHUFFLE, ST_BLOSC, ST_ADLER32, ST_FLETCHER32, ST_ZLIB, ST_BZ2 };
// the checksum stages strip 4 bytes in place; every other stage materialises its output in a slot pool
inline bool strips_only(StageKind k) { return k == ST_CRC32C || k == ST_ADLER32 || k == ST_FLETCHER32; }
inline StageKind checksum_stage(CodecKind k) {
  return k == CodecKind::Crc32c ? ST_CRC32C : k == CodecKind::Adler32 ? ST_ADLER32 : ST_FLETCHER32;
}
struct Stage {
  StageKind kind;
  int at_start = 0;
  uint32_t elementsize = 0;
  int pool = 0;  // destination slot pool for materialising stages
};

struct zgpu_plan {
  zgpu_ctx *ctx;   // holds a reference (dropped by the destructor)
  PoolBlocks mem;  // every device and pinned buffer below, for the plan's lifetime
  explicit zgpu_plan(zgpu_ctx *c) : ctx(c), mem(c) { ctx_ref(c); }
  std::mutex mu;  // one execute / status at a time per plan
  Lane own{};     // the plan's stream for executes without a caller stream (lazy)
  std::shared_ptr<Chain> chain;
  const Chain *leaf = nullptr;
  bool validate = true;
  uint32_t nd = 0;
  uint64_t n_desc = 0;
  uint32_t flags = 0;
  std::vector<uint64_t> out_shape;
  // host tables
  std::vector<ZgItem> items;
  std::vector<uint64_t> geom;
  std::vector<uint32_t> item_desc_status;  // plan-time per-desc status
  std::vector<ZgShard> shards;
  std::vector<Stage> stages;
  ZgScatter scatter{};
  uint32_t scatter_mode = SCATTER_GENERIC;
  uint64_t scatter_units = 0;
  bool sharded = false, nested = false;
  ZgIndexSpec ispec{}, ispec2{};  // ispec2: the middle shards' index (nested sharding)
  std::vector<ZgItem> mids;       // nested: one record per intersecting middle shard
  uint64_t slot_bytes = 0;
  int n_pools = 0;
  uint64_t alg_bytes_static = 0;  // decoded bytes written + (unsharded) encoded bytes + index bytes
  // device buffers
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
  ZstdScratch zs{};  // block-parallel zstd scratch (allocated when the chain has zstd)
  // side stream of the zstd sequence decoder (created on first use with the priority of the stream
  // the plan first runs on; ZGPU_ZSTD_FORK=0 keeps one stream)
  hipStream_t zside = nullptr;
  hipEvent_t zev[2] = {nullptr, nullptr};
  void zstd_fork(ZstdScratch &Z, hipStream_t s) {
    static const bool on = [] {
      const char *e = std::getenv("ZGPU_ZSTD_FORK");
      return !e || std::atoi(e) != 0;
    }();
    if (!on || (flags & ZGPU_ONE_STREAM)) return;
    if (!zside) {
      int prio = 0;
      if (s) (void)hipStreamGetPriority(s, &prio);
      HIPCHK(hipStreamCreateWithPriority(&zside, hipStreamNonBlocking, prio));
      for (hipEvent_t &e : zev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    Z.side = zside;
    Z.ev_fork = zev[0];
    Z.ev_join = zev[1];
  }
  // zstd in two pipelined halves (ZstdScratch::s2; blosc stream tables of many frames): opt-in with
  // ZGPU_ZSTD_SPLIT=1 (blosc-zstd bench 32.6 -> 35.6 ms with it: the halves' kernels contend more than
  // they overlap, profiles/r04an_zstd_split_ab.txt)
  hipStream_t zs2 = nullptr;
  hipEvent_t zev2[2] = {nullptr, nullptr};
  void zstd_split(ZstdScratch &Z, hipStream_t s) {
    const char *e = std::getenv("ZGPU_ZSTD_SPLIT");  // read per call (tests switch it)
    if (!e || std::atoi(e) == 0 || !Z.side) return;
    if (!zs2) {
      int prio = 0;
      if (s) (void)hipStreamGetPriority(s, &prio);
      HIPCHK(hipStreamCreateWithPriority(&zs2, hipStreamNonBlocking, prio));
      for (hipEvent_t &e : zev2) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    Z.s2 = zs2;
    Z.ev_half = zev2[0];
    Z.ev_done = zev2[1];
  }
  // blosc stage scratch (grown on demand; the stream table is sized from the frame headers)
  struct Grow {
    void *p = nullptr;
    size_t n = 0;
  };
  Grow bl_info, bl_bases, bl_subs, bl_sub_status, bl_sub_kind, bl_blocks, bl_tmp, bl_zblks, bl_znblk, bl_zmode,
      bl_zlit, bl_zseq, bl_zaux, bl_zser, bl_lzl, bl_zseg, bl_zrec, bl_zalias, bl_znorm, gz_crc, live_list,
      ck_parts;  // ck_parts: the adler32 / fletcher32 stages' range sums
  uint64_t in_len_hint = 0;  // the longest item before any stage, as far as the host knows: how many
                             // workgroups a checksum stage gives an item (k_linsum_strip), not its result
  uint8_t *bl_h = nullptr;  // pinned: BlInfo read-back (first execution)
  void *grow(Grow &g, size_t bytes) {
    if (g.n < bytes) {
      g.p = mem.regrow(g.p, bytes);
      g.n = bytes;
    }
    return g.p;
  }
  unsigned long long *d_counter = nullptr;
  // control block: [counter (256 B) | per-item status (4 B each)], cleared by ONE memset and read
  // back by ONE D2H copy into pinned memory (h_ctl) per execute
  uint8_t *d_ctl = nullptr, *h_ctl = nullptr;
  size_t ctl_bytes = 0;
  // A tiled plan whose every item is a whole chunk of full, 16-B aligned tiles scatters with
  // k_scatter_tiled_p (tiled_persistent_params; ZGPU_TILED_PERSIST=0: k_scatter_tiled): its constants
  // and the output element offset of each item's origin
  bool tiled_p = false;
  ZgTiledP tiled_q{};
  std::vector<uint64_t> origin;
  uint64_t *d_origin = nullptr;
  uint32_t last_path = SCATTER_GENERIC;  // zgpu_plan_scatter_path: of the last enqueue (before one: the plan's)
  uint64_t last_enc_bytes = 0;
  uint64_t last_counters[CTR_N] = {};
  uint8_t *last_out = nullptr;  // output of the last enqueue (a blosc layout overflow re-runs into it)
  BlCaps bl_caps{};             // blosc stream-table capacities recorded by the first execution
  bool bl_caps_valid = false, bl_caps_seen = false;
  bool bl_direct = false;  // the blosc stage may write whole chunks straight into the output (BlDecode::dout)
  bool gz_direct = false;  // the gzip stage may write whole chunks straight into the output (GzDirect)
  GzDirect gz{};
  // blosc as the last stage: per item the decoded byte range its selection needs ([0, max) for whole
  // chunks); blocks outside it are not decoded (blosc_decompress_bytes_partial)
  std::vector<uint64_t> bl_need;
  uint64_t *d_bl_need = nullptr;
  // zstd serial fallback: skipped once an execution of this plan had no serial item (a later one that
  // has some is re-run by plan_statuses with the fallback launched)
  bool zstd_serial_off = false, zstd_serial_skipped = false;
  uint32_t *d_zser = nullptr;
  uint32_t *d_order = nullptr;  // gzip stage: LPT dispatch order of the items
  uint32_t *d_gz_seg = nullptr;  // gzip stage: symbol-record scratch of the segmented decode
  uint64_t bz_rounds = 0;  // bz2 stage: rounds the last enqueue launched (ZGPU_CTR_BZ2_ROUNDS)
  Bz2Scratch bz{};  // bz2 stage: block records, BWT vectors and pre-RLE1 bytes of one round of items
  bool no_scatter = false;  // a whole-shard predecode plan: its bytes->bytes stages only (decode_general)

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
    if (zside) {
      (void)hipStreamSynchronize(zside);
      (void)hipStreamDestroy(zside);
    }
    if (zs2) {
      (void)hipStreamSynchronize(zs2);
      (void)hipStreamDestroy(zs2);
    }
    for (hipEvent_t e : zev2)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : zev)
      if (e) (void)hipEventDestroy(e);
    mem.release();
  }
};

// zgpu.cpp
void composed_axes(const Chain &c, uint32_t nd, uint32_t *m);
ZgIndexSpec index_spec(const Codec &sharding, uint64_t n_inner, bool validate);
zgpu_plan *plan_new(zgpu_ctx *ctx, const std::shared_ptr<Chain> &chain, bool validate, uint32_t nd,
                    const zgpu_chunk_desc *descs, uint64_t n, const uint64_t *out_shape, uint32_t flags);
void plan_upload(zgpu_plan &P, hipStream_t us);
void plan_enqueue(zgpu_plan &P, uint8_t *out, hipStream_t s);
int plan_statuses(zgpu_plan &P, int32_t *status, hipStream_t s);
hipStream_t pick_stream(Lane *L, void *s);
uint64_t volume(const uint64_t *shape, uint32_t nd);

struct CoBatch;
// zgpu_decode_pinned's result: a pooled pinned buffer of the context, or a slice of a coalesced
// batch's pack (the batch, and with it the pack, lives until every caller released its result)
struct zgpu_result {
  zgpu_ctx *ctx = nullptr;
  uint8_t *own = nullptr;             // pooled pinned buffer (uncoalesced call)
  std::shared_ptr<CoBatch> batch;     // coalesced call: the batch holding the pack
  ~zgpu_result() {
    if (own) ctx->host_free(own);
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
                               hipStream_t s);
#pragma GCC visibility pop
