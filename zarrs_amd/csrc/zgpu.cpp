// libzgpu: host orchestration of the MI355X chunk-decode pipeline behind the C ABI of include/zgpu.h --
// the calling thread's state (last error, counters, size detail), the C ABI, the decode call paths and
// the coalescer. The fused plan they run lives in plan_layout.cpp (host) and plan_exec.cpp (device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/zgpu.h"
#include "chain.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "kernels/launch.hpp"
#include "plan.hpp"
#include "fsstore.hpp"
#include "internal.hpp"
#include "xfer.hpp"

using namespace zgpu;

namespace {
thread_local std::string g_last_error;
thread_local uint64_t g_last_counters[CTR_N];
thread_local SizeDetail g_size_detail;
}  // namespace

int set_err(int st, const std::string &m) {
  g_last_error = m;
  return st;
}
SizeDetail &size_detail() { return g_size_detail; }
uint64_t *call_counters() { return g_last_counters; }

void zgpu::ctx_ref(zgpu_ctx *c) {
  if (c) c->refs.fetch_add(1, std::memory_order_relaxed);
}
void zgpu::ctx_unref(zgpu_ctx *c) {
  if (c && c->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete c;
}

static void reset_call_state() {
  for (uint64_t &c : g_last_counters) c = 0;
  g_size_detail = SizeDetail{};
}

int zgpu::set_last_error(int status, const std::string &msg) { return set_err(status, msg); }
zgpu_ctx *zgpu::chain_ctx(const zgpu_chain *c) { return c->ctx; }
const Chain &zgpu::chain_model(const zgpu_chain *c) { return *c->chain; }
bool zgpu::chain_validates(const zgpu_chain *c) { return c->validate; }
int zgpu::ctx_device(const zgpu_ctx *c) { return c->device; }
void *zgpu::ctx_dev_alloc(zgpu_ctx *c, size_t bytes) {  // nullptr on failure
  try {
    HIPCHK(hipSetDevice(c->device));
    return c->dev_alloc(bytes);
  } catch (const HipFail &) {
    return nullptr;
  }
}
void zgpu::ctx_dev_free(zgpu_ctx *c, void *p) { c->dev_free(p); }
hipStream_t zgpu::ctx_copy_stream(zgpu_ctx *c) {  // nullptr on failure
  std::lock_guard<std::mutex> lk(c->lane_mu);
  if (!c->peer && (hipSetDevice(c->device) != hipSuccess ||
                   hipStreamCreateWithFlags(&c->peer, hipStreamNonBlocking) != hipSuccess)) {
    c->peer = nullptr;
    return nullptr;
  }
  return c->peer;
}

static zgpu_plan *plan_new(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                           const uint64_t *out_shape, uint32_t flags) {
  return plan_new(ch->ctx, ch->chain, ch->validate, nd, descs, n, out_shape, flags);
}

void zgpu::begin_call() { reset_call_state(); }

int zgpu::plan_status_add(zgpu_plan *P, int32_t *status, void *stream, const uint64_t *desc_map) {
  ABI_GUARD_BEGIN
  if (!P) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  std::lock_guard<std::mutex> lk(P->mu);
  HIPCHK(hipSetDevice(P->ctx->device));
  const bool had_detail = g_size_detail.valid;
  const int rc = plan_statuses(*P, status, stream ? (hipStream_t)stream : plan_lane(*P)->stream);
  if (desc_map && !had_detail && g_size_detail.valid) g_size_detail.desc = desc_map[g_size_detail.desc];
  if (rc) set_err(rc, zgpu_status_name(rc));
  return rc;
  ABI_GUARD_END
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// array_read_ops_common.rs:20-109: subset -> intersecting chunks -> one descriptor per chunk, in
// C order of the chunk grid; lins[k] = descriptor k's C-order linear chunk-grid index.
// Returns ZGPU_OK, -1 for an empty subset (nothing to do), or an error status.
int zgpu::subset_descs(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                       const uint64_t *sel_start, const uint64_t *sel_shape, std::vector<zgpu_chunk_desc> &descs,
                       std::vector<uint64_t> &lins) {
  uint64_t grid[ZG_MAXD], lo[ZG_MAXD], hi[ZG_MAXD], idx[ZG_MAXD];
  uint64_t nchunks = 1;
  bool empty = false;
  for (uint32_t d = 0; d < nd; d++) {
    if (chunk_shape[d] == 0) return set_err(ZGPU_INVALID_ARGUMENT, "zero chunk extent");
    if (sel_start[d] + sel_shape[d] > array_shape[d])
      return set_err(ZGPU_INVALID_ARGUMENT, "array subset out of bounds");
    grid[d] = (array_shape[d] + chunk_shape[d] - 1) / chunk_shape[d];
    if (sel_shape[d] == 0) {
      empty = true;
      continue;
    }
    lo[d] = sel_start[d] / chunk_shape[d];
    hi[d] = (sel_start[d] + sel_shape[d] - 1) / chunk_shape[d] + 1;
    nchunks *= hi[d] - lo[d];
    idx[d] = lo[d];
  }
  if (empty) return -1;
  descs.reserve(nchunks);
  lins.reserve(nchunks);
  for (;;) {
    zgpu_chunk_desc D{};
    uint64_t lin = 0;
    for (uint32_t d = 0; d < nd; d++) {
      lin = lin * grid[d] + idx[d];
      const uint64_t cs = idx[d] * chunk_shape[d], ce = cs + chunk_shape[d];
      const uint64_t s0 = std::max(sel_start[d], cs), s1 = std::min(sel_start[d] + sel_shape[d], ce);
      D.chunk_shape[d] = chunk_shape[d];
      D.sel_start[d] = s0 - cs;
      D.sel_shape[d] = s1 - s0;
      D.out_start[d] = s0 - sel_start[d];
    }
    descs.push_back(D);
    lins.push_back(lin);
    int d = (int)nd - 1;
    for (; d >= 0; d--) {
      if (++idx[d] < hi[d]) break;
      idx[d] = lo[d];
    }
    if (d < 0) break;
  }
  return ZGPU_OK;
}

extern "C" {

const char *zgpu_version(void) { return "zgpu 0.1.0 (gfx950)"; }

const char *zgpu_status_name(int s) {
  static const char *names[] = {"OK", "INVALID_CHECKSUM", "DECODED_SIZE_MISMATCH", "SHARD_INDEX_OOB",
                                "CORRUPT_STREAM", "INVALID_BYTE_RANGE", "UNSUPPORTED", "CRC_INPUT_TOO_SHORT",
                                "SHARD_TOO_SMALL", "SHUFFLE_LENGTH", "INVALID_ARGUMENT", "HIP_ERROR",
                                "STORAGE_ERROR", "CAST_NOT_REPRESENTABLE"};
  return (s >= 0 && s <= 13) ? names[s] : "UNKNOWN";
}

const char *zgpu_last_error(const zgpu_ctx *) { return g_last_error.c_str(); }

int zgpu_ctx_create(int dev, zgpu_ctx **out) {
  ABI_GUARD_BEGIN
  if (!out) return set_err(ZGPU_INVALID_ARGUMENT, "out is NULL");
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (dev < 0 || dev >= n) return set_err(ZGPU_INVALID_ARGUMENT, "no such HIP device");
  HIPCHK(hipSetDevice(dev));
  auto c = std::make_unique<zgpu_ctx>();
  c->device = dev;
  if (const char *e = std::getenv("ZGPU_CTX_LANES")) c->max_lanes = (uint32_t)std::max(1, std::min(64, std::atoi(e)));
  if (const char *e = std::getenv("ZGPU_POOL_CAP_MB")) c->pool_cap = (size_t)std::max(64, std::atoi(e)) << 20;
  if (const char *e = std::getenv("ZGPU_PINNED_CAP_MB")) c->host_cap = (size_t)std::max(64, std::atoi(e)) << 20;
  c->release_lane(c->acquire_lane());  // the first lane up front (stream creation errors surface here)
  *out = c.release();
  return ZGPU_OK;
  ABI_GUARD_END
}

void zgpu_ctx_destroy(zgpu_ctx *c) { ctx_unref(c); }

int64_t zgpu_ctx_refcount(const zgpu_ctx *c) { return c ? c->refs.load() : 0; }

int zgpu_ctx_pool_stats(const zgpu_ctx *c, uint64_t *dev_live, uint64_t *dev_free, uint64_t *host_live,
                        uint64_t *host_free) {
  if (!c) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  zgpu_ctx *m = const_cast<zgpu_ctx *>(c);  // the allocator lock only
  std::lock_guard<std::mutex> lk(m->mu);
  uint64_t dl = 0, hl = 0, hf = 0;
  for (const auto &kv : c->live_dev) dl += kv.second;
  for (const auto &kv : c->live_host) hl += kv.second;
  hf = c->free_host_bytes;
  if (dev_live) *dev_live = dl;
  if (dev_free) *dev_free = c->free_dev_bytes;
  if (host_live) *host_live = hl;
  if (host_free) *host_free = hf;
  return ZGPU_OK;
}

int zgpu_ctx_release_cached(zgpu_ctx *c) {
  if (!c) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) (void)hipGetLastError();
  c->trim_free_locked(0);
  c->trim_host_locked(0);
  (void)hipGetLastError();
  return ZGPU_OK;
}

int zgpu_chain_create(zgpu_ctx *ctx, const char *codecs_json, const char *data_type, const void *fill,
                      uint32_t fill_len, int validate, zgpu_chain **out) {
  ABI_GUARD_BEGIN
  if (!ctx || !codecs_json || !data_type || !out) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  uint32_t es, comp;
  if (!data_type_info(data_type, es, comp)) return set_err(ZGPU_UNSUPPORTED, std::string("data type ") + data_type);
  if (fill && fill_len != es) return set_err(ZGPU_INVALID_ARGUMENT, "fill_len != element size");
  uint8_t f[16] = {0};
  if (fill) std::memcpy(f, fill, es);
  Json j = Json::parse(codecs_json);
  auto ch = std::make_unique<zgpu_chain>();
  ch->chain = parse_chain(j, data_type, f);
  ch->validate = validate != 0;
  ctx_ref(ctx);
  ch->ctx = ctx;
  *out = ch.release();
  return ZGPU_OK;
  ABI_GUARD_END
}

void zgpu_chain_destroy(zgpu_chain *c) {
  if (!c) return;
  zgpu_ctx *ctx = c->ctx;
  delete c;
  ctx_unref(ctx);
}

uint32_t zgpu_chain_element_size(const zgpu_chain *c) { return c ? c->chain->es : 0; }

int zgpu_plan_create(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n, const uint64_t *out_shape,
                     uint32_t flags, zgpu_plan **out) {
  ABI_GUARD_BEGIN
  if (!ch || !out || !out_shape || (n && !descs)) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  if (!(flags & ZGPU_ENC_DEVICE)) return set_err(ZGPU_INVALID_ARGUMENT, "plans need device-resident inputs");
  HIPCHK(hipSetDevice(ch->ctx->device));
  LaneScope ls(ch->ctx);
  std::unique_ptr<zgpu_plan> P(plan_new(ch, nd, descs, n, out_shape, flags));
  plan_upload(*P, ls.L->stream);
  HIPCHK(hipStreamSynchronize(ls.L->stream));
  *out = P.release();
  return ZGPU_OK;
  ABI_GUARD_END
}

int zgpu_plan_execute(zgpu_plan *P, void *out, int32_t *status, void *stream) {
  ABI_GUARD_BEGIN
  if (!P || !out) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  std::lock_guard<std::mutex> lk(P->mu);
  HIPCHK(hipSetDevice(P->ctx->device));
  hipStream_t s = pick_stream(plan_lane(*P), stream);
  reset_call_state();
  plan_enqueue(*P, (uint8_t *)out, s);
  if (!status) return ZGPU_OK;
  return plan_statuses(*P, status, s);
  ABI_GUARD_END
}

// A status call is a call of its own: the thread's counters and size-mismatch detail are this plan's
// last execute's alone, whatever another plan's status call (or a second one of this plan) left there.
int zgpu_plan_status(zgpu_plan *P, int32_t *status, void *stream) {
  reset_call_state();
  return plan_status_add(P, status, stream, nullptr);
}

void zgpu_plan_destroy(zgpu_plan *P) {
  if (!P) return;
  { std::lock_guard<std::mutex> lk(P->mu); }  // no execute of it still running on another thread
  delete P;
}

uint32_t zgpu_plan_scatter_path(const zgpu_plan *P) { return P ? P->last_path : ZGPU_SCATTER_GENERIC; }

uint64_t zgpu_plan_algorithmic_bytes(const zgpu_plan *P) { return P ? P->L.alg_bytes_static + P->last_enc_bytes : 0; }

uint32_t zgpu_plan_counters(const zgpu_plan *P, uint64_t *out, uint32_t n) {
  if (!P || !out) return 0;
  const uint32_t k = std::min<uint32_t>(n, CTR_N);
  std::memcpy(out, P->last_counters, k * sizeof(uint64_t));
  return k;
}

int zgpu_last_size_mismatch(uint64_t *desc, uint64_t *len, uint64_t *expected_len) {
  if (!g_size_detail.valid) return 0;
  if (desc) *desc = g_size_detail.desc;
  if (len) *len = g_size_detail.len;
  if (expected_len) *expected_len = g_size_detail.expected;
  return 1;
}

uint32_t zgpu_last_counters(uint64_t *out, uint32_t n) {
  if (!out) return 0;
  const uint32_t k = std::min<uint32_t>(n, CTR_N);
  std::memcpy(out, g_last_counters, k * sizeof(uint64_t));
  return k;
}

// Host input and host output, both pinned, descriptors covering the whole output: the batch is cut
// into sub-batches of whole axis-0 row ranges (no descriptor straddles a cut), and sub-batch k's H2D
// (copy stream 0), decode (s) and D2H of its rows (copy stream 1) overlap with its neighbours' --
// PCIe is full duplex, so the host-to-host rate approaches the one-direction bound instead of half
// of it. Returns false (nothing done) when the batch does not cut into at least two sub-batches.
static bool decode_pipelined(zgpu_chain *ch, Lane *LN, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                             uint8_t *out, const uint64_t *out_shape, uint32_t flags, int32_t *status, hipStream_t s,
                             int &rc) {
  constexpr uint64_t K = 16;  // target sub-batches
  zgpu_ctx *C = ch->ctx;
  uint64_t row_bytes = ch->chain->es;
  for (uint32_t d = 1; d < nd; d++) row_bytes *= out_shape[d];
  std::vector<uint64_t> ord(n);
  for (uint64_t i = 0; i < n; i++) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
    return descs[a].out_start[0] != descs[b].out_start[0] ? descs[a].out_start[0] < descs[b].out_start[0] : a < b;
  });
  struct Group { uint64_t b, e, r0, r1; };
  std::vector<Group> groups;
  const uint64_t rows_per = std::max<uint64_t>(1, (out_shape[0] + K - 1) / K);
  uint64_t reach = 0, gb = 0, gr = 0;
  for (uint64_t k = 0; k < n; k++) {
    const zgpu_chunk_desc &d = descs[ord[k]];
    if (k > gb && d.out_start[0] >= reach && d.out_start[0] - gr >= rows_per) {
      groups.push_back(Group{gb, k, gr, d.out_start[0]});
      gb = k;
      gr = d.out_start[0];
    }
    reach = std::max<uint64_t>(reach, d.out_start[0] + d.sel_shape[0]);
  }
  if (groups.empty() || gr != groups.back().r1 || reach != out_shape[0]) return false;
  groups.push_back(Group{gb, n, gr, reach});
  if (groups.front().r0 != 0) return false;
  for (hipStream_t &cs : LN->copy)
    if (!cs) HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  // encoded bytes: per sub-batch, address-sorted and merged ranges in one device staging buffer
  std::vector<size_t> range_of(n, SIZE_MAX);  // descriptor -> its merged range in its sub-batch
  std::vector<std::vector<HostRange>> granges(groups.size());
  uint64_t total = 0;
  for (size_t g = 0; g < groups.size(); g++) {
    std::vector<uint64_t> idx(ord.begin() + groups[g].b, ord.begin() + groups[g].e);
    std::sort(idx.begin(), idx.end(),
              [&](uint64_t a, uint64_t b) { return (uintptr_t)descs[a].enc < (uintptr_t)descs[b].enc; });
    std::vector<HostRange> &R = granges[g];
    for (uint64_t i : idx) {
      if (!descs[i].enc || !descs[i].enc_len) continue;
      const uint8_t *p = (const uint8_t *)descs[i].enc;
      if (!R.empty() && p <= R.back().src + R.back().len) {
        HostRange &r = R.back();
        const uint64_t end = std::max<uint64_t>((uint64_t)(p - r.src) + descs[i].enc_len, r.len);
        total += end - r.len;
        r.len = end;
      } else {
        total = (total + 255) & ~(uint64_t)255;
        R.push_back(HostRange{p, descs[i].enc_len, total});
        total += descs[i].enc_len;
      }
      range_of[i] = R.size() - 1;
    }
  }
  Scratch sc(C, s);
  uint8_t *enc_dev = sc.dev<uint8_t>(total ? total : 1);
  uint8_t *dout = sc.dev<uint8_t>(out_shape[0] * row_bytes);
  struct Events {  // destroyed after the plans below, before the buffers above go back
    std::vector<hipEvent_t> v;
    ~Events() {
      for (hipEvent_t e : v)
        if (e) (void)hipEventDestroy(e);
    }
  } events{std::vector<hipEvent_t>(2 * groups.size(), nullptr)};
  std::vector<hipEvent_t> &ev = events.v;
  std::vector<std::unique_ptr<zgpu_plan>> plans(groups.size());
  try {
    for (hipEvent_t &e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (size_t g = 0; g < groups.size(); g++) {
      const Group &G = groups[g];
      for (const HostRange &r : granges[g])
        HIPCHK(hipMemcpyAsync(enc_dev + r.dev_off, r.src, r.len, hipMemcpyHostToDevice, LN->copy[0]));
      HIPCHK(hipEventRecord(ev[2 * g], LN->copy[0]));
      std::vector<zgpu_chunk_desc> gd;
      gd.reserve(G.e - G.b);
      for (uint64_t k = G.b; k < G.e; k++) {
        const uint64_t i = ord[k];
        zgpu_chunk_desc d = descs[i];
        const size_t r = range_of[i];
        if (r != SIZE_MAX) {
          const HostRange &hr = granges[g][r];
          d.enc = enc_dev + hr.dev_off + ((const uint8_t *)descs[i].enc - hr.src);
        } else {
          d.enc = nullptr;
        }
        gd.push_back(d);
      }
      plans[g].reset(plan_new(ch, nd, gd.data(), gd.size(), out_shape, flags | ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE));
      plan_upload(*plans[g], s);
      HIPCHK(hipStreamWaitEvent(s, ev[2 * g], 0));
      plan_enqueue(*plans[g], dout, s);
      HIPCHK(hipEventRecord(ev[2 * g + 1], s));
      HIPCHK(hipStreamWaitEvent(LN->copy[1], ev[2 * g + 1], 0));
      HIPCHK(hipMemcpyAsync(out + G.r0 * row_bytes, dout + G.r0 * row_bytes, (G.r1 - G.r0) * row_bytes,
                            hipMemcpyDeviceToHost, LN->copy[1]));
    }
    std::vector<int32_t> all(n, 0);
    for (size_t g = 0; g < groups.size(); g++) {
      const Group &G = groups[g];
      std::vector<int32_t> st(G.e - G.b, 0);
      plan_statuses(*plans[g], st.data(), s);
      for (uint64_t k = G.b; k < G.e; k++) all[ord[k]] = st[k - G.b];
    }
    rc = 0;  // the first failing descriptor in the caller's order
    for (uint64_t i = 0; i < n; i++) {
      if (status) status[i] = all[i];
      if (!rc) rc = all[i];
    }
    HIPCHK(hipStreamSynchronize(LN->copy[1]));
  } catch (...) {
    (void)hipDeviceSynchronize();  // the copy streams too
    throw;
  }
  return true;
}

}  // extern "C"

// Host inputs -> one device staging buffer: chunks sorted by address and touching / overlapping ones
// merged into ranges; pinned ranges are DMA'd directly (one copy per range), pageable ones through
// the pinned staging slabs. local[i].enc is rewritten to descriptor i's device copy.
struct HostStage {
  Scratch sc;  // the staging buffer and slabs, and the call's other temporaries on the same stream
  uint8_t *enc = nullptr, *pin = nullptr;
  static constexpr uint64_t slab = 64ull << 20;
  HostStage(zgpu_ctx *c, hipStream_t s) : sc(c, s) {}
  uint8_t *stage() {  // 2 slabs of pinned staging, only for pageable host buffers
    if (!pin) pin = sc.pinned<uint8_t>(2 * slab);
    return pin;
  }
};

static void stage_host_inputs(HostStage &H, const zgpu_chunk_desc *descs, uint64_t n,
                              std::vector<zgpu_chunk_desc> &local, hipStream_t s) {
  local.assign(descs, descs + n);
  std::vector<uint64_t> order;
  for (uint64_t i = 0; i < n; i++)
    if (descs[i].enc && descs[i].enc_len) order.push_back(i);
  std::sort(order.begin(), order.end(),
            [&](uint64_t a, uint64_t b) { return (uintptr_t)descs[a].enc < (uintptr_t)descs[b].enc; });
  std::vector<HostRange> ranges;
  std::vector<uint64_t> range_of(n, 0);
  uint64_t total = 0;
  for (uint64_t i : order) {
    const uint8_t *p = (const uint8_t *)descs[i].enc;
    if (!ranges.empty() && p <= ranges.back().src + ranges.back().len) {
      HostRange &r = ranges.back();
      const uint64_t end = std::max<uint64_t>((uint64_t)(p - r.src) + descs[i].enc_len, r.len);
      total += end - r.len;
      r.len = end;
    } else {
      total = (total + 255) & ~(uint64_t)255;
      ranges.push_back(HostRange{p, descs[i].enc_len, total});
      total += descs[i].enc_len;
    }
    range_of[i] = ranges.size() - 1;
  }
  if (!total) return;
  H.enc = H.sc.dev<uint8_t>(total);
  bool pinned = true;
  for (const HostRange &r : ranges)
    if (!host_is_pinned(r.src) || !host_is_pinned(r.src + r.len - 1)) {
      pinned = false;
      break;
    }
  HIPCHK(h2d_ranges(H.enc, ranges, pinned, pinned ? nullptr : H.stage(), HostStage::slab, host_copy_threads(), s));
  for (uint64_t i : order) {
    const HostRange &r = ranges[range_of[i]];
    local[i].enc = H.enc + r.dev_off + ((const uint8_t *)descs[i].enc - r.src);
  }
}

static uint64_t covered_volume(const zgpu_chunk_desc *descs, uint64_t n, uint32_t nd) {
  uint64_t covered = 0;
  for (uint64_t i = 0; i < n; i++) covered += sel_volume(descs[i], nd);
  return covered;
}

uint64_t volume(const uint64_t *shape, uint32_t nd) {
  uint64_t v = 1;
  for (uint32_t d = 0; d < nd; d++) v *= shape[d];
  return v;
}

// Device-side decode of descriptors whose encoded bytes are on the device into dout (out_shape):
// the general decode, per-descriptor statuses, first failing descriptor as the return value.
static int decode_device(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *dd, uint64_t n, uint8_t *dout,
                         const uint64_t *out_shape, uint32_t flags, int32_t *status, hipStream_t s) {
  GeneralCall G{ch->ctx, ch->validate && !(flags & ZGPU_NO_VALIDATE), nd, dout, out_shape,
                flags | ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE, s, {}};
  std::vector<int32_t> st(n, 0);
  decode_general(G, ch->chain, dd, n, st.data());
  int rc = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (status) status[i] = st[i];
    if (!rc) rc = st[i];
  }
  return rc;
}

// zgpu_decode_batch / zgpu_decode_into on one lane (LN, stream s): every output form.
static int decode_call(zgpu_chain *ch, Lane *LN, hipStream_t s, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                       const zgpu_out_view &V, uint32_t flags, int32_t *status) {
  zgpu_ctx *C = ch->ctx;
  const uint32_t es = ch->chain->es;
  const bool whole = box_is_whole(nd, V.array_shape, V.start, V.shape);
  const uint64_t out_elems = volume(V.shape, nd);
  const bool fused = fused_plannable(*ch->chain) && uniform_shapes(descs, n, nd);
  if (!(flags & ZGPU_ENC_DEVICE) && !(flags & ZGPU_OUT_DEVICE) && n >= 2 && fused && whole) {
    // pinned host in and out, full coverage: the overlapped sub-batch pipeline
    const uint64_t out_b = out_elems * es;
    bool pinned = out_b && host_is_pinned(V.base) && host_is_pinned((const uint8_t *)V.base + out_b - 1);
    for (uint64_t i = 0; i < n && pinned; i++) {
      const uint8_t *e = (const uint8_t *)descs[i].enc;
      if (e && descs[i].enc_len && (!host_is_pinned(e) || !host_is_pinned(e + descs[i].enc_len - 1))) pinned = false;
    }
    int rc = 0;
    if (pinned && covered_volume(descs, n, nd) == out_elems &&
        decode_pipelined(ch, LN, nd, descs, n, (uint8_t *)V.base, V.shape, flags, status, s, rc))
      return rc;
  }
  HostStage H(C, s);
  std::vector<zgpu_chunk_desc> local;
  const zgpu_chunk_desc *dd = descs;
  if (!(flags & ZGPU_ENC_DEVICE)) {
    stage_host_inputs(H, descs, n, local, s);
    dd = local.data();
  }
  if (flags & ZGPU_OUT_DEVICE) {
    if (whole) return decode_device(ch, nd, dd, n, (uint8_t *)V.base, V.shape, flags, status, s);
    // a window of a device array: decoded in place through the whole array's strides (descriptors
    // shifted by the window origin; one outside its window fails alone, as it would against out_shape)
    std::vector<zgpu_chunk_desc> sub;
    std::vector<uint64_t> owner;
    std::vector<int32_t> st(n, 0);
    for (uint64_t i = 0; i < n; i++) {
      if (!desc_geometry_ok(dd[i], nd, V.shape)) {
        st[i] = ZGPU_INVALID_ARGUMENT;
        continue;
      }
      zgpu_chunk_desc d = dd[i];
      for (uint32_t k = 0; k < nd; k++) d.out_start[k] += V.start[k];
      sub.push_back(d);
      owner.push_back(i);
    }
    std::vector<int32_t> sst(sub.size(), 0);
    decode_device(ch, nd, sub.data(), sub.size(), (uint8_t *)V.base, V.array_shape, flags, sst.data(), s);
    if (g_size_detail.valid) g_size_detail.desc = owner[g_size_detail.desc];
    for (size_t k = 0; k < sub.size(); k++) st[owner[k]] = sst[k];
    int rc = 0;
    for (uint64_t i = 0; i < n; i++) {
      if (status) status[i] = st[i];
      if (!rc) rc = st[i];
    }
    return rc;
  }
  // host output: decoded into a compact device copy of the window, copied back box-wise; parts of the
  // window no descriptor covers keep the caller's bytes (the regions are disjoint,
  // ArrayBytesFixedDisjointView, so equal volumes mean full coverage and no upload)
  const uint64_t out_bytes = out_elems * es;
  uint8_t *dout = H.sc.dev<uint8_t>(out_bytes ? out_bytes : 1);
  const BoxRuns R = box_runs(nd, V.array_shape, V.start, V.shape, es);
  if (covered_volume(descs, n, nd) != out_elems)
    HIPCHK(h2d_box(R, dout, (const uint8_t *)V.base, H.stage(), HostStage::slab, host_copy_threads(), s));
  const int rc = decode_device(ch, nd, dd, n, dout, V.shape, flags, status, s);
  HIPCHK(d2h_box(R, (uint8_t *)V.base, dout, H.stage(), HostStage::slab, host_copy_threads(), s));
  return rc;
}

// ------------------------------------------------------------------------------------------------
// Coalescing of concurrent host-in / host-out calls (ZGPU_COALESCE). zarrs' read path calls the codec
// once per shard (or chunk) from each rayon worker (array_read_ops_common.rs:173-176,
// sharding_codec.rs:617-707), and one shard's inner chunks fill a few percent of the GPU's decode
// waves. Calls on one chain that arrive within the collect window become ONE batch: the first caller
// (the batch's leader) waits for the window to close (or the batch to fill), stacks every caller's
// window along axis 0 of one device output (trailing axes padded to the largest), uploads all
// encoded bytes in one packed H2D, decodes everything in one launch sequence, packs the windows
// compactly on the device (k_box_copy) and copies them back in one D2H into pinned memory. Every
// caller then places its own window's rows into its host array (in parallel) and returns its own
// statuses. Batches of one context run concurrently, each on a lane of its own.
// ------------------------------------------------------------------------------------------------
struct CoCall {
  zgpu_chain *ch;
  uint32_t nd;
  const zgpu_chunk_desc *descs;
  uint64_t n;
  zgpu_out_view V;
  uint32_t flags;
  int32_t *status;
  uint64_t enc_bytes = 0;
  // results, set by the leader
  bool done = false, call_error = false;  // call_error: the batch failed as a whole (rc, err)
  int rc = 0;
  std::string err;
  SizeDetail sd;
  uint64_t pack_off = 0;  // byte offset of this caller's compact window in the batch's host pack
};

struct CoBatch {
  zgpu_ctx *C = nullptr;
  std::vector<CoCall *> calls;
  uint64_t bytes = 0;
  bool closed = false;
  std::condition_variable cv;
  uint8_t *pack = nullptr;  // pinned: every caller's window, compact, back to back
  uint64_t id = 0;          // trace id
  ~CoBatch() {
    if (pack) C->host_free(pack);
  }
};

struct CoKey {
  zgpu_chain *ch;
  uint32_t flags, nd;
  bool operator<(const CoKey &o) const {
    return ch != o.ch ? ch < o.ch : flags != o.flags ? flags < o.flags : nd < o.nd;
  }
};

struct Coalescer {
  std::mutex mu;
  std::map<CoKey, std::shared_ptr<CoBatch>> open;
  uint32_t window_us = 200, max_calls = 8;
  uint64_t max_bytes = 1ull << 30;
  uint64_t batches = 0, calls = 0, seq = 0;
  uint64_t active = 0;  // coalescable calls inside coalesced_call (under mu)
  // Batches decoding at once (under mu): a leader waits for a slot while its batch keeps taking
  // joiners. Each batch is a synchronous H2D -> decode -> D2H chain on its lane; with more of them than
  // the process's HIP hardware queues (4 by default) their kernels queue behind each other, and a few
  // larger batches fill the GPU better (drop-in sweep, profiles/r05/r05d8_dropin_rect_pack_inflight_cap.txt).
  uint32_t max_inflight = 3, inflight = 0;
  std::condition_variable slot_cv;
};

// ZGPU_TRACE=1: one stderr line per coalesced-batch phase (microseconds since the first trace)
static bool co_tracing() {
  static const bool on = [] {
    const char *e = std::getenv("ZGPU_TRACE");
    return e && std::atoi(e) != 0;
  }();
  return on;
}
static void co_trace(const char *what, uint64_t batch, uint64_t a = 0, uint64_t b = 0) {
  if (!co_tracing()) return;
  static const auto t0 = std::chrono::steady_clock::now();
  const long long us =
      std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  std::fprintf(stderr, "[zgpu-trace] %lld %s %llu %llu %llu\n", us, what, (unsigned long long)batch,
               (unsigned long long)a, (unsigned long long)b);
}

static Coalescer &coalescer(zgpu_ctx *C) {
  std::lock_guard<std::mutex> lk(C->mu);
  if (!C->co) {
    C->co = new Coalescer();
    if (const char *e = std::getenv("ZGPU_COALESCE_US")) C->co->window_us = (uint32_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("ZGPU_COALESCE_CALLS")) C->co->max_calls = (uint32_t)std::max(1, std::atoi(e));
    if (const char *e = std::getenv("ZGPU_COALESCE_BYTES")) C->co->max_bytes = std::strtoull(e, nullptr, 10);
    if (const char *e = std::getenv("ZGPU_CO_INFLIGHT")) C->co->max_inflight = (uint32_t)std::max(1, std::atoi(e));
  }
  return *C->co;
}

// The leader's work: one decode of every caller's descriptors; fills each call's results and the
// batch's host pack.
static void co_run(CoBatch &B, Lane *LN) {
  zgpu_ctx *C = B.C;
  CoCall &c0 = *B.calls[0];
  zgpu_chain *ch = c0.ch;
  const uint32_t nd = c0.nd, es = ch->chain->es;
  HIPCHK(hipSetDevice(C->device));
  hipStream_t s = pick_stream(LN, nullptr);
  // stacked output: caller k's window at rows [row0[k], row0[k] + V.shape[0]) of axis 0
  uint64_t stacked[ZG_MAXD] = {0};
  std::vector<uint64_t> row0(B.calls.size());
  for (size_t k = 0; k < B.calls.size(); k++) {
    const zgpu_out_view &V = B.calls[k]->V;
    row0[k] = stacked[0];
    stacked[0] += V.shape[0];
    for (uint32_t d = 1; d < nd; d++) stacked[d] = std::max(stacked[d], V.shape[d]);
  }
  std::vector<zgpu_chunk_desc> all;
  std::vector<std::pair<uint32_t, uint64_t>> owner;  // (call, descriptor)
  std::vector<std::vector<int32_t>> st(B.calls.size());
  for (size_t k = 0; k < B.calls.size(); k++) {
    CoCall &c = *B.calls[k];
    st[k].assign(c.n, 0);
    for (uint64_t i = 0; i < c.n; i++) {
      if (!desc_geometry_ok(c.descs[i], nd, c.V.shape)) {
        st[k][i] = ZGPU_INVALID_ARGUMENT;
        continue;
      }
      zgpu_chunk_desc d = c.descs[i];
      d.out_start[0] += row0[k];
      all.push_back(d);
      owner.push_back({(uint32_t)k, i});
    }
  }
  HostStage H(C, s);
  struct Drain {  // the pack and D2H below move to the high-priority stream: s is then that one, and a
    hipStream_t &s;  // failure must not return dout / dpack (H's) with work still queued on it
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  std::vector<zgpu_chunk_desc> local;
  co_trace("batch-start", B.id, B.calls.size(), all.size());
  stage_host_inputs(H, all.data(), all.size(), local, s);
  co_trace("h2d-done", B.id);
  uint64_t row_elems = 1;
  for (uint32_t d = 1; d < nd; d++) row_elems *= stacked[d];
  const uint64_t stacked_bytes = stacked[0] * row_elems * es;
  uint64_t pack_bytes = 0;
  for (CoCall *c : B.calls) {
    c->pack_off = pack_bytes;
    pack_bytes += volume(c->V.shape, nd) * es;
  }
  uint8_t *dout = H.sc.dev<uint8_t>(stacked_bytes ? stacked_bytes : 1);
  std::vector<int32_t> ast(all.size(), 0);
  decode_device(ch, nd, local.data(), local.size(), dout, stacked, c0.flags, ast.data(), s);
  co_trace("decode-done", B.id);
  const SizeDetail sd = g_size_detail;
  for (size_t j = 0; j < all.size(); j++) st[owner[j].first][owner[j].second] = ast[j];
  if (sd.valid && sd.desc < owner.size()) {
    CoCall &c = *B.calls[owner[sd.desc].first];
    c.sd = sd;
    c.sd.desc = owner[sd.desc].second;
  }
  // The pack kernels and the D2H run on a high-priority stream: the other lanes' decodes hold the
  // CUs with long-running waves, and a normal-priority pack kernel queued behind them waited for
  // their slots (trace: 60 MB packs taking 20+ ms). ZGPU_CO_HIPRIO=0: the lane's own stream.
  static const bool hiprio = [] {
    const char *e = std::getenv("ZGPU_CO_HIPRIO");
    return !e || std::atoi(e) != 0;
  }();
  if (hiprio) {
    if (!LN->out_hi) {
      int least = 0, greatest = 0;
      HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIPCHK(hipStreamCreateWithPriority(&LN->out_hi, hipStreamNonBlocking, greatest));
    }
    HIPCHK(hipStreamSynchronize(s));  // (decode_device has read its statuses back: a no-op)
    s = LN->out_hi;
  }
  // pack: a window whose trailing extents are the stacked ones is already compact in place
  bool compact = true;
  for (CoCall *c : B.calls)
    for (uint32_t d = 1; d < nd; d++)
      if (c->V.shape[d] != stacked[d]) compact = false;
  std::vector<BoxRuns> boxes;
  bool rect = false;  // every window a 3-D box: packed by the copy engines, no kernel
  if (!compact) {
    static const bool rect_on = [] {
      const char *e = std::getenv("ZGPU_CO_PACK_RECT");
      return !e || std::atoi(e) != 0;
    }();
    rect = rect_on;
    for (size_t k = 0; k < B.calls.size(); k++) {
      uint64_t org[ZG_MAXD] = {0};
      org[0] = row0[k];
      boxes.push_back(box_runs(nd, stacked, org, B.calls[k]->V.shape, es));
      if (boxes.back().outer > 2) rect = false;
    }
  }
  // power-of-two size classes (>= 64 MiB): batches of varying size reuse pooled pinned buffers
  // instead of page-locking new ones
  if (compact || rect) co_trace("packed", B.id, compact ? 0 : 2);
  uint64_t cls = 64ull << 20;
  while (cls < pack_bytes) cls <<= 1;
  B.pack = (uint8_t *)C->host_alloc(cls);
  co_trace("pack-alloc", B.id);
  if (compact) {
    if (pack_bytes) HIPCHK(hipMemcpyAsync(B.pack, dout, pack_bytes, hipMemcpyDeviceToHost, s));
  } else if (rect) {
    // Each caller's window straight from the stacked output into its place in the pinned pack as
    // one pitched 3-D copy (DMA): a box-copy kernel queued while other lanes' decode waves hold the
    // CUs waited for their slots (trace: pack median 5 ms at 8 lanes, 20 ms at 2 lanes with bigger
    // batches), and the copy engines need none.
    for (size_t k = 0; k < B.calls.size(); k++) {
      const BoxRuns &R = boxes[k];
      if (!R.n_runs) continue;
      const uint64_t w = R.run_bytes;
      const uint64_t h = R.outer >= 1 ? R.shape[R.outer - 1] : 1, depth = R.outer >= 2 ? R.shape[0] : 1;
      const uint64_t pitch = R.outer >= 1 ? R.stride[R.outer - 1] : w;
      const uint64_t sy = R.outer >= 2 ? R.stride[0] / pitch : h;
      hipMemcpy3DParms p3{};
      p3.srcPtr = make_hipPitchedPtr(dout + R.base, pitch, w, sy);
      p3.dstPtr = make_hipPitchedPtr(B.pack + B.calls[k]->pack_off, w, w, h);
      p3.extent = make_hipExtent(w, h, depth);
      p3.kind = hipMemcpyDeviceToHost;
      HIPCHK(hipMemcpy3DAsync(&p3, s));
    }
  } else {
    uint8_t *dpack = H.sc.dev<uint8_t>(pack_bytes ? pack_bytes : 1);
    for (size_t k = 0; k < B.calls.size(); k++) {
      const BoxRuns &R = boxes[k];
      ZgBoxCopy P{};
      P.outer = R.outer;
      for (uint32_t d = 0; d < R.outer; d++) {
        P.shape[d] = R.shape[d];
        P.src_stride[d] = R.stride[d];
      }
      uint64_t cs = R.run_bytes;  // compact strides of the outer axes
      for (int d = (int)R.outer - 1; d >= 0; d--) {
        P.dst_stride[d] = cs;
        cs *= R.shape[d];
      }
      P.src_base = R.base;
      P.dst_base = B.calls[k]->pack_off;
      P.run_bytes = R.run_bytes;
      P.n_runs = R.n_runs;
      HIPCHK(launch_box_copy(dout, dpack, P, s));
    }
    if (co_tracing()) {
      HIPCHK(hipStreamSynchronize(s));
      co_trace("packed", B.id, 1);
    }
    if (pack_bytes) HIPCHK(hipMemcpyAsync(B.pack, dpack, pack_bytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  co_trace("d2h-done", B.id, pack_bytes);
  for (size_t k = 0; k < B.calls.size(); k++) {
    CoCall &c = *B.calls[k];
    c.rc = 0;
    for (uint64_t i = 0; i < c.n; i++) {
      if (c.status) c.status[i] = st[k][i];
      if (!c.rc) c.rc = st[k][i];
    }
  }
}

// A caller's encoded bytes copied into pinned memory by the caller's own thread before it joins a
// batch: a batch's callers pack their inputs in parallel (each on its own thread, overlapping the
// other lanes' GPU work) and the leader's upload is one DMA per contiguous range, instead of the
// leader staging every caller's pageable bytes itself. Ranges (descriptors sorted by address, touching
// ones merged) are placed back to back; local[i].enc points into the pinned copy. Returns nullptr
// (local untouched) when there is nothing to copy or the bytes are pinned already.
static uint8_t *pin_caller_inputs(PoolBlocks &mem, const zgpu_chunk_desc *descs, uint64_t n,
                                  std::vector<zgpu_chunk_desc> &local) {
  std::vector<uint64_t> order;
  for (uint64_t i = 0; i < n; i++)
    if (descs[i].enc && descs[i].enc_len) order.push_back(i);
  if (order.empty()) return nullptr;
  std::sort(order.begin(), order.end(),
            [&](uint64_t a, uint64_t b) { return (uintptr_t)descs[a].enc < (uintptr_t)descs[b].enc; });
  std::vector<HostRange> ranges;
  std::vector<uint64_t> range_of(n, 0);
  uint64_t total = 0;
  for (uint64_t i : order) {
    const uint8_t *p = (const uint8_t *)descs[i].enc;
    if (!ranges.empty() && p <= ranges.back().src + ranges.back().len) {
      HostRange &r = ranges.back();
      const uint64_t end = std::max<uint64_t>((uint64_t)(p - r.src) + descs[i].enc_len, r.len);
      total += end - r.len;
      r.len = end;
    } else {
      ranges.push_back(HostRange{p, descs[i].enc_len, total});
      total += descs[i].enc_len;
    }
    range_of[i] = ranges.size() - 1;
  }
  bool pinned = true;
  for (const HostRange &r : ranges)
    if (!host_is_pinned(r.src) || !host_is_pinned(r.src + r.len - 1)) {
      pinned = false;
      break;
    }
  if (pinned) return nullptr;
  uint64_t cls = 4ull << 20;  // power-of-two classes: the pooled buffers are reused call after call
  while (cls < total) cls <<= 1;
  uint8_t *pin = mem.pinned<uint8_t>(cls);
  std::vector<uint8_t *> d;
  std::vector<const uint8_t *> sp;
  std::vector<uint64_t> ln;
  for (const HostRange &r : ranges) {
    d.push_back(pin + r.dev_off);
    sp.push_back(r.src);
    ln.push_back(r.len);
  }
  parallel_memcpy(d, sp, ln, 2);
  local.assign(descs, descs + n);
  for (uint64_t i : order) {
    const HostRange &r = ranges[range_of[i]];
    local[i].enc = pin + r.dev_off + ((const uint8_t *)descs[i].enc - r.src);
  }
  return pin;
}

static int coalesced_call(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                          const zgpu_out_view &V, uint32_t flags, int32_t *status,
                          zgpu_result **keep = nullptr, const void **keep_data = nullptr) {
  zgpu_ctx *C = ch->ctx;
  Coalescer &K = coalescer(C);
  static const bool pin_in = [] {
    const char *e = std::getenv("ZGPU_CO_PIN");
    return !e || std::atoi(e) != 0;
  }();
  std::vector<zgpu_chunk_desc> pinned_descs;
  PoolBlocks pin_mem(C);  // pinned host memory the batch's H2D reads: this call outlives its batch's run
  const uint8_t *pin = pin_in ? pin_caller_inputs(pin_mem, descs, n, pinned_descs) : nullptr;
  co_trace("pinned", 0, pin ? 1 : 0);
  if (pin) descs = pinned_descs.data();
  CoCall me{ch, nd, descs, n, V, flags, status};
  for (uint64_t i = 0; i < n; i++)
    if (descs[i].enc) me.enc_bytes += descs[i].enc_len;
  const CoKey key{ch, flags, nd};
  std::shared_ptr<CoBatch> B;
  bool leader = false;
  std::unique_lock<std::mutex> lk(K.mu);
  K.active++;  // left below, once this call's batch is done (the lock is held there)
  auto it = K.open.find(key);
  if (it == K.open.end()) {
    B = std::make_shared<CoBatch>();
    B->C = C;
    B->id = ++K.seq;
    K.open[key] = B;
    leader = true;
  } else {
    B = it->second;
  }
  B->calls.push_back(&me);
  B->bytes += me.enc_bytes;
  co_trace(leader ? "arrive-lead" : "arrive-join", B->id, me.enc_bytes);
  auto close = [&]() {
    B->closed = true;
    auto jt = K.open.find(key);
    if (jt != K.open.end() && jt->second == B) K.open.erase(jt);
  };
  if (B->calls.size() >= K.max_calls || B->bytes >= K.max_bytes) {
    close();
    B->cv.notify_all();
  }
  if (leader) {
    // the batch takes joiners for the collect window, and then for as long as its leader waits for a
    // free lane: under load (every lane decoding an earlier batch) batches grow by themselves. A lone
    // caller (no other coalescable call in flight on the context) does not wait: a single-threaded
    // reader pays no collect window per chunk.
    if (K.active > 1)
      B->cv.wait_until(lk, std::chrono::steady_clock::now() + std::chrono::microseconds(K.window_us),
                       [&] { return B->closed; });
    K.slot_cv.wait(lk, [&] { return K.inflight < K.max_inflight; });
    K.inflight++;
    lk.unlock();
    int rc = 0;
    std::string err;
    Lane *LN = nullptr;
    try {
      HIPCHK(hipSetDevice(C->device));
      LN = C->acquire_lane();
    } catch (const HipFail &e) {
      rc = ZGPU_HIP_ERROR;
      err = std::string(e.what) + ": " + hipGetErrorString(e.e);
    }
    co_trace("lane", B->id);
    lk.lock();
    if (!B->closed) close();
    K.batches++;
    K.calls += B->calls.size();
    lk.unlock();
    if (!rc) try {
      co_run(*B, LN);
    } catch (const ChainError &e) {
      rc = e.status;
      err = e.msg;
    } catch (const HipFail &e) {
      rc = ZGPU_HIP_ERROR;
      err = std::string(e.what) + ": " + hipGetErrorString(e.e);
    } catch (const std::exception &e) {
      rc = ZGPU_INVALID_ARGUMENT;
      err = e.what();
    }
    if (LN) C->release_lane(LN);
    lk.lock();
    K.inflight--;
    K.slot_cv.notify_one();
    for (CoCall *c : B->calls) {
      if (rc) {
        c->rc = rc;
        c->err = err;
        c->call_error = true;
        c->sd = SizeDetail{};
      }
      c->done = true;
    }
    B->cv.notify_all();
  } else {
    B->cv.wait(lk, [&] { return me.done; });
  }
  K.active--;
  lk.unlock();
  g_size_detail = me.sd;
  if (me.call_error) return set_err(me.rc, me.err);
  if (keep) {  // zgpu_decode_pinned: the caller copies its compact window out of the pack itself
    auto *R = new zgpu_result();
    ctx_ref(C);
    R->ctx = C;
    R->batch = B;
    *keep = R;
    *keep_data = B->pack + me.pack_off;
    if (me.rc) set_err(me.rc, zgpu_status_name(me.rc));
    return me.rc;
  }
  // this caller's window: its rows placed from the pinned pack by this caller's own thread (the
  // batch's callers do this in parallel)
  const BoxRuns R = box_runs(nd, V.array_shape, V.start, V.shape, ch->chain->es);
  const uint64_t nb = R.n_runs * R.run_bytes;
  // the batch's callers place their rows concurrently; each takes its share of the copy threads
  const int share = std::max<int>(1, host_copy_threads() / (int)std::max<size_t>(1, B->calls.size()));
  copy_box_runs(R, (uint8_t *)V.base, B->pack + me.pack_off, 0, nb, true, std::min(share, 4));
  co_trace("copied-out", B->id, nb);
  if (me.rc) set_err(me.rc, zgpu_status_name(me.rc));
  return me.rc;
}

static int decode_entry(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                        const zgpu_out_view &V, uint32_t flags, int32_t *status, void *stream) {
  zgpu_ctx *C = ch->ctx;
  for (uint32_t d = 0; d < nd; d++)
    if (V.start[d] + V.shape[d] > V.array_shape[d]) return set_err(ZGPU_INVALID_ARGUMENT, "view outside its array");
  HIPCHK(hipSetDevice(C->device));
  reset_call_state();
  if ((flags & ZGPU_COALESCE) && !(flags & (ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE)) && n &&
      covered_volume(descs, n, nd) == volume(V.shape, nd))
    return coalesced_call(ch, nd, descs, n, V, flags & ~ZGPU_COALESCE, status);
  LaneScope ls(C);
  hipStream_t s = pick_stream(ls.L, stream);
  const int rc = decode_call(ch, ls.L, s, nd, descs, n, V, flags & ~ZGPU_COALESCE, status);
  if (rc) set_err(rc, zgpu_status_name(rc));
  return rc;
}

void delete_coalescer(Coalescer *co) { delete co; }

extern "C" {

int zgpu_decode_pinned(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n, const uint64_t *out_shape,
                       uint32_t flags, int32_t *status, const void **data, zgpu_result **result) {
  ABI_GUARD_BEGIN
  if (data) *data = nullptr;
  if (result) *result = nullptr;
  if (!ch || !out_shape || (n && !descs) || !data || !result) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  if (flags & (ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE))
    return set_err(ZGPU_INVALID_ARGUMENT, "zgpu_decode_pinned takes host inputs and returns host memory");
  zgpu_ctx *C = ch->ctx;
  HIPCHK(hipSetDevice(C->device));
  reset_call_state();
  const uint64_t bytes = volume(out_shape, nd) * ch->chain->es;
  if ((flags & ZGPU_COALESCE) && n && covered_volume(descs, n, nd) == volume(out_shape, nd)) {
    zgpu_out_view V{};
    V.base = nullptr;  // never written: the result stays in the pack
    for (uint32_t d = 0; d < nd; d++) V.array_shape[d] = V.shape[d] = out_shape[d];
    zgpu_result *R = nullptr;
    const void *p = nullptr;
    const int rc = coalesced_call(ch, nd, descs, n, V, flags & ~ZGPU_COALESCE, status, &R, &p);
    if (rc) {
      delete R;
      return rc;
    }
    *result = R;
    *data = p;
    return ZGPU_OK;
  }
  // one call: its own pooled pinned buffer (pinned host output takes the overlapped D2H paths)
  std::unique_ptr<zgpu_result> R(new zgpu_result());
  ctx_ref(C);
  R->ctx = C;
  R->own = (uint8_t *)C->host_alloc(bytes ? bytes : 1);
  zgpu_out_view V{};
  V.base = R->own;
  for (uint32_t d = 0; d < nd; d++) V.array_shape[d] = V.shape[d] = out_shape[d];
  if (covered_volume(descs, n, nd) != volume(out_shape, nd) && bytes)  // parts no descriptor covers: zero
    std::memset(R->own, 0, bytes);
  LaneScope ls(C);
  hipStream_t s = pick_stream(ls.L, nullptr);
  const int rc = decode_call(ch, ls.L, s, nd, descs, n, V, flags & ~ZGPU_COALESCE, status);
  if (rc) return set_err(rc, zgpu_status_name(rc));
  *data = R->own;
  *result = R.release();
  return ZGPU_OK;
  ABI_GUARD_END
}

void zgpu_result_release(zgpu_result *r) { delete r; }

int zgpu_decode_batch(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n, void *out,
                      const uint64_t *out_shape, uint32_t flags, int32_t *status, void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !out_shape || (n && !descs) || !out) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  zgpu_out_view V{};
  V.base = out;
  for (uint32_t d = 0; d < nd; d++) V.array_shape[d] = V.shape[d] = out_shape[d];
  return decode_entry(ch, nd, descs, n, V, flags, status, stream);
  ABI_GUARD_END
}

int zgpu_decode_into(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n, const zgpu_out_view *view,
                     uint32_t flags, int32_t *status, void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !view || (n && !descs) || !view->base) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  return decode_entry(ch, nd, descs, n, *view, flags, status, stream);
  ABI_GUARD_END
}

int zgpu_ctx_set_coalescing(zgpu_ctx *ctx, uint32_t window_us, uint32_t max_calls, uint64_t max_bytes) {
  if (!ctx) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  Coalescer &K = coalescer(ctx);
  std::lock_guard<std::mutex> lk(K.mu);
  K.window_us = window_us;
  K.max_calls = std::max<uint32_t>(1, max_calls);
  K.max_bytes = max_bytes ? max_bytes : UINT64_MAX;
  return ZGPU_OK;
}

int zgpu_ctx_coalescing_stats(const zgpu_ctx *ctx, uint64_t *batches, uint64_t *calls) {
  if (!ctx) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  Coalescer &K = coalescer(const_cast<zgpu_ctx *>(ctx));
  std::lock_guard<std::mutex> lk(K.mu);
  if (batches) *batches = K.batches;
  if (calls) *calls = K.calls;
  return ZGPU_OK;
}

int zgpu_retrieve_array_subset(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                               const void *const *chunk_ptrs, const uint64_t *chunk_lens, const uint64_t *sel_start,
                               const uint64_t *sel_shape, void *out, uint32_t flags, void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !array_shape || !chunk_shape || !chunk_ptrs || !chunk_lens || !sel_start || !sel_shape || !out)
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  std::vector<zgpu_chunk_desc> descs;
  std::vector<uint64_t> lins;
  const int r = subset_descs(nd, array_shape, chunk_shape, sel_start, sel_shape, descs, lins);
  if (r) return r < 0 ? ZGPU_OK : r;
  for (size_t k = 0; k < descs.size(); k++) {
    descs[k].enc = chunk_ptrs[lins[k]];
    descs[k].enc_len = descs[k].enc ? chunk_lens[lins[k]] : 0;
  }
  return zgpu_decode_batch(ch, nd, descs.data(), descs.size(), out, sel_shape, flags, nullptr, stream);
  ABI_GUARD_END
}

// Filesystem store -> HBM -> decode, pipelined over sub-batches in descriptor order: host threads
// read sub-batch g into pinned slab g%2 (positional reads, O_DIRECT pages with ZGPU_DIRECT_IO) while
// sub-batch g-1's H2D (copy stream 0) and decode (the call's stream) run; slab g%2 is reused once
// sub-batch g-2's H2D has completed.
int zgpu_decode_files(zgpu_chain *ch, uint32_t nd, const zgpu_chunk_desc *descs, const zgpu_file_range *files,
                      uint64_t n, void *out, const uint64_t *out_shape, uint32_t flags, int32_t *status,
                      void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !out_shape || (n && (!descs || !files)) || !out) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  zgpu_ctx *C = ch->ctx;
  HIPCHK(hipSetDevice(C->device));
  LaneScope ls(C);
  Lane *LN = ls.L;
  hipStream_t s = pick_stream(LN, stream);
  reset_call_state();
  const int threads = host_copy_threads();
  std::vector<FileRange> fr(n);
  for (uint64_t i = 0; i < n; i++) {
    fr[i].path = files[i].path;
    fr[i].offset = files[i].offset;
    fr[i].len = files[i].len;
  }
  struct Closer {
    std::vector<FileRange> &r;
    ~Closer() { fs_close_all(r); }
  } closer{fr};
  std::string err = fs_open_all(fr, (flags & ZGPU_DIRECT_IO) != 0, threads);
  if (!err.empty()) return set_err(ZGPU_STORAGE_ERROR, err);
  // sub-batches: ~8 of them, 32-512 MiB of reads each
  auto readable = [&](uint64_t i) { return !fr[i].missing && !fr[i].bad_range; };
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; i++)
    if (readable(i)) total += (fr[i].rd_len + 4095) & ~(uint64_t)4095;
  uint64_t target = std::min<uint64_t>(512ull << 20, std::max<uint64_t>(32ull << 20, total / 8));
  if (const char *e = std::getenv("ZGPU_FS_GROUP_BYTES")) target = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
  struct Group { uint64_t b, e, base, bytes; };
  std::vector<Group> groups;
  {
    Group g{0, 0, 0, 0};
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t sz = readable(i) ? ((fr[i].rd_len + 4095) & ~(uint64_t)4095) : 0;
      if (i > g.b && g.bytes + sz > target) {
        g.e = i;
        groups.push_back(g);
        g = Group{i, 0, g.base + g.bytes, 0};
      }
      fr[i].slab_off = g.bytes;  // page-aligned (O_DIRECT buffers)
      g.bytes += sz;
    }
    g.e = n;
    if (n) groups.push_back(g);
  }
  uint64_t max_g = 4096;
  for (const Group &g : groups) max_g = std::max(max_g, g.bytes);
  uint64_t out_elems = 1;
  for (uint32_t d = 0; d < nd; d++) out_elems *= out_shape[d];
  const uint64_t out_bytes = out_elems * ch->chain->es;
  const bool host_out = !(flags & ZGPU_OUT_DEVICE);
  for (hipStream_t &cs : LN->copy)
    if (!cs) HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  Scratch sc(C, s);  // declared first: returned after cleanup() below drained the streams
  uint8_t *enc_dev = nullptr, *dout = (uint8_t *)out, *slab[2] = {nullptr, nullptr}, *pin_stage = nullptr;
  const uint64_t stage_slab = 64ull << 20;
  std::vector<hipEvent_t> ev(groups.size(), nullptr);
  std::vector<std::unique_ptr<zgpu_plan>> plans(groups.size());
  auto cleanup = [&]() {
    (void)hipStreamSynchronize(LN->copy[0]);
    (void)hipStreamSynchronize(s);
    plans.clear();
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  };
  int rc = 0;
  const bool fused = fused_plannable(*ch->chain) && uniform_shapes(descs, n, nd);
  std::vector<int32_t> all(n, 0);
  try {
    enc_dev = sc.dev<uint8_t>(total ? total : 1);
    if (host_out) {
      dout = sc.dev<uint8_t>(out_bytes ? out_bytes : 1);
      uint64_t covered = 0;  // disjoint regions: equal volumes mean full coverage (no upload)
      for (uint64_t i = 0; i < n; i++) {
        uint64_t v = 1;
        for (uint32_t d = 0; d < nd; d++) v *= descs[i].sel_shape[d];
        covered += v;
      }
      if (covered != out_elems) {
        pin_stage = sc.pinned<uint8_t>(2 * stage_slab);
        HIPCHK(h2d_bytes(dout, (const uint8_t *)out, out_bytes, pin_stage, stage_slab, threads, s));
      }
    }
    for (int k = 0; k < 2 && k < (int)groups.size(); k++) slab[k] = sc.pinned<uint8_t>(max_g);
    for (hipEvent_t &e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (size_t g = 0; g < groups.size(); g++) {
      const Group &G = groups[g];
      if (g >= 2) HIPCHK(hipEventSynchronize(ev[g - 2]));  // slab g%2 free again
      uint8_t *sl = slab[g & 1];
      std::vector<uint64_t> idx;
      for (uint64_t i = G.b; i < G.e; i++)
        if (readable(i)) idx.push_back(i);
      err = fs_read_into(fr, idx, sl, threads);
      if (!err.empty()) throw ChainError{ZGPU_STORAGE_ERROR, err};
      if (G.bytes) HIPCHK(hipMemcpyAsync(enc_dev + G.base, sl, G.bytes, hipMemcpyHostToDevice, LN->copy[0]));
      HIPCHK(hipEventRecord(ev[g], LN->copy[0]));
      std::vector<zgpu_chunk_desc> gd(descs + G.b, descs + G.e);
      for (uint64_t i = G.b; i < G.e; i++) {
        zgpu_chunk_desc &d = gd[i - G.b];
        if (readable(i)) {  // an empty object still has a (valid) address
          d.enc = enc_dev + G.base + fr[i].slab_off + (fr[i].offset - fr[i].rd_off);
          d.enc_len = fr[i].len;
        } else {
          d.enc = nullptr;
          d.enc_len = 0;
        }
      }
      if (!fused) {  // the general decode is synchronous: this group is done before the next is read
        HIPCHK(hipStreamWaitEvent(s, ev[g], 0));
        GeneralCall GC{C, ch->validate && !(flags & ZGPU_NO_VALIDATE), nd, dout, out_shape,
                       flags | ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE, s, {}};
        decode_general(GC, ch->chain, gd.data(), gd.size(), all.data() + G.b);
        continue;
      }
      plans[g].reset(plan_new(ch, nd, gd.data(), gd.size(), out_shape, flags | ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE));
      plan_upload(*plans[g], s);
      HIPCHK(hipStreamWaitEvent(s, ev[g], 0));
      plan_enqueue(*plans[g], dout, s);
    }
    for (size_t g = 0; g < groups.size(); g++)
      if (plans[g]) plan_statuses(*plans[g], all.data() + groups[g].b, s);
    for (uint64_t i = 0; i < n; i++) {
      if (fr[i].bad_range) all[i] = ZGPU_INVALID_BYTE_RANGE;
      if (status) status[i] = all[i];
      if (!rc) rc = all[i];
    }
    if (host_out) {
      if (!pin_stage) pin_stage = sc.pinned<uint8_t>(2 * stage_slab);
      HIPCHK(d2h_bytes((uint8_t *)out, dout, out_bytes, pin_stage, stage_slab, threads, s));
    }
  } catch (...) {
    cleanup();
    throw;
  }
  cleanup();
  if (rc) set_err(rc, zgpu_status_name(rc));
  return rc;
  ABI_GUARD_END
}

int zgpu_retrieve_array_subset_files(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape,
                                     const uint64_t *chunk_shape, const char *const *chunk_paths,
                                     const uint64_t *sel_start, const uint64_t *sel_shape, void *out, uint32_t flags,
                                     void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !array_shape || !chunk_shape || !chunk_paths || !sel_start || !sel_shape || !out)
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  std::vector<zgpu_chunk_desc> descs;
  std::vector<uint64_t> lins;
  const int r = subset_descs(nd, array_shape, chunk_shape, sel_start, sel_shape, descs, lins);
  if (r) return r < 0 ? ZGPU_OK : r;
  std::vector<zgpu_file_range> files(descs.size());
  for (size_t k = 0; k < descs.size(); k++) files[k] = zgpu_file_range{chunk_paths[lins[k]], 0, UINT64_MAX};
  return zgpu_decode_files(ch, nd, descs.data(), files.data(), descs.size(), out, sel_shape, flags, nullptr, stream);
  ABI_GUARD_END
}

}  // extern "C"
