// libzgpu: a fused decode plan on the device.
//
// A batch of chunk descriptors is planned on the host into leaf work items (a plain chunk, or one
// inner chunk of a shard that intersects the selection), uploaded once, and decoded by a short
// sequence of batched kernels, each over ALL items of the batch:
//   [sharded]  k_shard_index (index chain decode + crc32c verify per shard)
//              k_item_resolve (index lookup per item: byte range, empty -> fill, out-of-bounds)
//   b2b stages in reverse metadata order (codec_chain.rs:612-617):
//              crc32c verify+strip (pointer arithmetic, no copy) | gzip | zstd | unshuffle
//   final      fused bytes(endian) + transpose + (innermost shuffle) + scatter/fill into the output
// Per-item statuses come back in one D2H copy; the first failing item of a descriptor gives that
// descriptor's status (try_for_each semantics, sharding_codec.rs:702-704).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "plan.hpp"

using namespace zgpu;

// Sizes the zstd scratch of n items of slot_bytes (zstd_scratch_sizes) and binds it to Z: alloc(k, bytes)
// gives buffer k of ZSTD_SCRATCH_BUFFERS (bytes > 0). A buffer the sizes leave out stays null.
template <class Alloc>
static void zstd_bind(ZstdScratch &Z, uint64_t n, uint64_t slot_bytes, const ZstdWants &wants, Alloc alloc) {
  const ZstdScratchSizes S = zstd_scratch_sizes(n, slot_bytes, device_cu_count(), wants);
  auto get = [&](int k, auto *&p, uint64_t bytes) { p = bytes ? (decltype(+p))alloc(k, bytes) : nullptr; };
  Z.blk_cap = S.blk_cap, Z.lit_stride = S.lit_stride, Z.seq_cap = S.seq_cap, Z.lit_rec_wgs = S.lit_rec_wgs;
  get(0, Z.blks, S.blks);
  get(1, Z.norm, S.norm);
  get(2, Z.nblk, S.nblk);
  get(3, Z.mode, S.mode);
  get(4, Z.lit, S.lit);
  get(5, Z.seq, S.seq);
  get(6, Z.ser_list, S.ser_list);
  get(7, Z.lit_rec, S.lit_rec);
  get(8, Z.alias, S.alias);
  get(9, Z.ext, S.ext);
  get(ZSTD_SCRATCH_BUFFERS - 1, Z.ext_cnt, S.ext_cnt);
}

void plan_upload(zgpu_plan &P, hipStream_t us) {
  const size_t ni = P.L.items.size();
  if (ni) {
    P.d_items = P.mem.dev<ZgItem>(ni);
    P.d_items_init = P.mem.dev<ZgItem>(ni);
    P.d_geom = P.mem.dev<uint64_t>(P.L.geom.size());
    HIPCHK(hipMemcpyAsync(P.d_items_init, P.L.items.data(), ni * sizeof(ZgItem), hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(P.d_geom, P.L.geom.data(), P.L.geom.size() * 8, hipMemcpyHostToDevice, us));
    for (int k = 0; k < P.L.n_pools; k++) P.d_pool[k] = P.mem.dev<uint8_t>(ni * P.L.slot_bytes);
    if (!P.L.bl_need.empty()) {
      P.blosc.d_need = P.mem.dev<uint64_t>(P.L.bl_need.size());
      HIPCHK(hipMemcpyAsync(P.blosc.d_need, P.L.bl_need.data(), P.L.bl_need.size() * 8, hipMemcpyHostToDevice, us));
    }
    for (const Stage &s : P.L.stages) {
      if ((s.kind == ST_GZIP || s.kind == ST_ZLIB) && !P.gzip.d_order) {
        P.gzip.d_order = P.mem.dev<uint32_t>(ni);
        if (const uint64_t b = gzip_seg_scratch_bytes((uint32_t)ni)) P.gzip.d_seg = (uint32_t *)P.mem.dev<uint8_t>(b);
      }
      if (s.kind == ST_BZ2 && !P.bz2.bz.base) {
        // 5 x slot_bytes of BWT vector (+ 1.25 x of bytes before RLE1, + block records) per item: a batch
        // whose scratch passes the budget (ZGPU_BZ2_SCRATCH_MB, read per plan; default 8192) runs in rounds
        P.bz2.bz.item_bytes = bz2_item_scratch_bytes(P.L.slot_bytes, P.bz2.bz.cap, P.bz2.bz.tt_cap);
        const char *e = std::getenv("ZGPU_BZ2_SCRATCH_MB");
        const uint64_t mb = e ? std::strtoull(e, nullptr, 10) : 0;
        const uint64_t budget = (mb ? mb : 8192) << 20;
        uint64_t per_round = std::max<uint64_t>(1, budget / P.bz2.bz.item_bytes);
        per_round = std::min<uint64_t>(per_round, std::max<uint64_t>(1, (1u << 30) / P.bz2.bz.cap));
        P.bz2.bz.round_items = (uint32_t)std::min<uint64_t>(per_round, ni);
        const uint64_t items_bytes = P.bz2.bz.round_items * P.bz2.bz.item_bytes;  // a multiple of 256
        P.bz2.bz.base = P.mem.dev<uint8_t>(items_bytes + bz2_list_bytes(P.bz2.bz.round_items, P.bz2.bz.cap));
        P.bz2.bz.lists = (uint32_t *)(P.bz2.bz.base + items_bytes);
      }
      if (s.kind == ST_ZSTD && !P.zstd.zs.blks)  // (the latency mode: a plan's own stage, few frames)
        zstd_bind(P.zstd.zs, ni, P.L.slot_bytes, ZstdWants{false, true, zstd_knobs_from_env()},
                  [&](int, uint64_t bytes) { return P.mem.dev<uint8_t>(bytes); });
    }
  }
  // the longest encoded item: known for plain chunks; an inner chunk's length comes from its shard's
  // index on the device, so the chain's bound stands in for it (no more than the longest shard)
  P.in_len_hint = 0;
  if (P.L.sharded) {
    uint64_t shard_max = 0;
    for (const ZgShard &sh : P.L.shards) shard_max = std::max(shard_max, sh.len);
    const int64_t b = P.L.leaf ? chain_encoded_bound(*P.L.leaf, P.L.scatter.nelem) : -1;
    P.in_len_hint = b >= 0 ? std::min<uint64_t>((uint64_t)b, shard_max) : shard_max;
  } else {
    for (const ZgItem &it : P.L.items) P.in_len_hint = std::max(P.in_len_hint, it.len);
  }
  // one scratch for every checksum stage of the plan, sized for the longest input any of them can be
  // given a hint of (the stages run one after another on the plan's stream)
  for (const Stage &s : P.L.stages)
    if (ni && (s.kind == ST_ADLER32 || s.kind == ST_FLETCHER32))
      P.grow(P.ck_parts, linsum_scratch_bytes((uint32_t)ni, std::max(P.in_len_hint, P.L.slot_bytes)));
  P.ctl_bytes = 256 + ni * 4;
  P.d_ctl = P.mem.dev<uint8_t>(P.ctl_bytes);
  P.h_ctl = P.mem.pinned<uint8_t>(P.ctl_bytes);
  if (P.L.tiled_p) {
    P.d_origin = P.mem.dev<uint64_t>(ni);
    HIPCHK(hipMemcpyAsync(P.d_origin, P.L.origin.data(), ni * 8, hipMemcpyHostToDevice, us));
  }
  P.d_counter = (unsigned long long *)P.d_ctl;
  P.d_status = (uint32_t *)(P.d_ctl + 256);
  P.zstd.zs.counters = P.d_counter + CTR_ZSTD_SERIAL;
  P.zstd.zs.lat_count = P.d_counter + CTR_ZSTD_LATENCY;
  P.zstd.zs.ser_count = P.d_counter + CTR_ZSTD_NSER;
  P.zstd.zs.max_nblk = P.d_counter + CTR_ZSTD_MAXBLK;
  if (!P.L.shards.empty()) {
    P.d_shards = P.mem.dev<ZgShard>(P.L.shards.size());
    P.d_index = P.mem.dev<uint64_t>(P.L.shards.size() * P.L.ispec.n_inner * 2);
    P.d_shard_status = P.mem.dev<uint32_t>(P.L.shards.size());
    HIPCHK(hipMemcpyAsync(P.d_shards, P.L.shards.data(), P.L.shards.size() * sizeof(ZgShard), hipMemcpyHostToDevice,
                          us));
  }
  if (!P.L.mids.empty()) {
    const size_t nm = P.L.mids.size();
    P.d_mids = P.mem.dev<ZgItem>(nm);
    P.d_mids_init = P.mem.dev<ZgItem>(nm);
    P.d_mid_status = P.mem.dev<uint32_t>(nm);
    P.d_shard_status2 = P.mem.dev<uint32_t>(nm);
    P.d_mid_shards = P.mem.dev<ZgShard>(nm);
    P.d_index2 = P.mem.dev<uint64_t>(nm * P.L.ispec2.n_inner * 2);
    HIPCHK(hipMemcpyAsync(P.d_mids_init, P.L.mids.data(), nm * sizeof(ZgItem), hipMemcpyHostToDevice, us));
  }
}

// blosc stage: frame headers -> stream table layout -> streams + blocks on the device -> zstd / lz4 /
// blosclz stream decode -> per-block gather + unshuffle into the item slots. The first execution of a
// plan reads the headers back to size the table (the one host round trip of any stage) and records
// the sizes as capacities; later executions lay the table out on the device against them
// (k_blosc_layout) and stay asynchronous. A later input that outgrows them is re-run by plan_statuses.
static void blosc_stage(zgpu_plan &P, const Stage &st, uint8_t *out, hipStream_t s) {
  const uint32_t ni = (uint32_t)P.L.items.size();
  uint8_t *dst = P.d_pool[st.pool];
  BlInfo *info = (BlInfo *)P.grow(P.blosc.info, ni * sizeof(BlInfo));
  HIPCHK(launch_blosc_info(P.d_items, P.d_status, ni, P.L.slot_bytes, info, s));
  uint64_t *d_bases = (uint64_t *)P.grow(P.blosc.bases, ni * 16);
  BlDecode D{};
  D.bases = d_bases;
  if (P.L.bl_direct && ((uintptr_t)out & 15) == 0) {
    D.dout = out;
    D.geom = P.d_geom;
    D.sc = P.L.scatter;
  }
  D.ovf = P.d_counter + CTR_BLOSC_OVF;
  D.need = P.blosc.d_need;
  D.blocks_decoded = P.d_counter + CTR_BLOSC_BLOCKS;
  BlCaps &caps = P.blosc.caps;
  const bool cached = P.blosc.caps_valid;
  if (!cached) {
    if (!P.blosc.h) P.blosc.h = (uint8_t *)P.mem.pinned<BlInfo>(ni);  // (a plan's item count is fixed)
    HIPCHK(hipMemcpyAsync(P.blosc.h, info, ni * sizeof(BlInfo), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<BlInfo> hi(ni);
    std::memcpy(hi.data(), P.blosc.h, ni * sizeof(BlInfo));
    BlCaps exact{0, 0, 0, 0};
    for (uint32_t i = 0; i < ni; i++) {
      if (hi[i].comp == BL_COMP_SKIP) continue;
      exact.n_sub += hi[i].nsub;
      exact.n_blk += hi[i].nblk;
      if (hi[i].nsub)
        exact.kinds |= hi[i].comp == BL_COMP_ZSTD ? BL_HAS_ZSTD : hi[i].comp == BL_COMP_LZ4 ? BL_HAS_LZ4
                       : hi[i].comp == BL_COMP_BLOSCLZ ? BL_HAS_BLOSCLZ : hi[i].comp == BL_COMP_ZLIB ? BL_HAS_ZLIB
                       : hi[i].comp == BL_COMP_SNAPPY ? BL_HAS_SNAPPY : 0u;
      exact.max_ne = std::max<uint64_t>(exact.max_ne, hi[i].max_ne);
    }
    // capacities only grow (a plan whose inputs alternate between layouts settles on their maximum)
    if (P.blosc.caps_seen) {
      caps.n_sub = std::max(caps.n_sub, exact.n_sub);
      caps.n_blk = std::max(caps.n_blk, exact.n_blk);
      caps.max_ne = std::max(caps.max_ne, exact.max_ne);
      caps.kinds |= exact.kinds;
    } else {
      caps = exact;
    }
    P.blosc.caps_seen = P.blosc.caps_valid = true;
  }
  D.n_sub = caps.n_sub;
  D.n_blk = caps.n_blk;
  D.n_zstd = caps.kinds & BL_HAS_ZSTD;
  D.n_lz4 = caps.kinds & BL_HAS_LZ4;
  D.n_blosclz = caps.kinds & BL_HAS_BLOSCLZ;
  D.n_zlib = caps.kinds & BL_HAS_ZLIB;
  D.n_snappy = caps.kinds & BL_HAS_SNAPPY;
  const uint64_t ns = std::max<uint64_t>(D.n_sub, 1);
  D.subs = (ZgItem *)P.grow(P.blosc.subs, ns * sizeof(ZgItem));
  D.sub_status = (uint32_t *)P.grow(P.blosc.sub_status, ns * 4);
  D.sub_kind = (uint32_t *)P.grow(P.blosc.sub_kind, ns * 4);
  D.blocks = (BlBlock *)P.grow(P.blosc.blocks, std::max<uint64_t>(D.n_blk, 1) * sizeof(BlBlock));
  if (D.n_zstd + D.n_lz4 + D.n_blosclz + D.n_zlib + D.n_snappy) {
    D.sub_slot = (caps.max_ne + 255) & ~(uint64_t)255;
    D.tmp = (uint8_t *)P.grow(P.blosc.tmp, D.n_sub * D.sub_slot);
  }
  if (D.n_zlib) {
    D.zaux = (uint2 *)P.grow(P.blosc.zaux, D.n_sub * sizeof(uint2));
    if (const uint64_t b = gzip_seg_scratch_bytes((uint32_t)D.n_sub)) D.zseg = (uint32_t *)P.grow(P.blosc.zseg, b);
  }
  D.lz_list = (D.n_lz4 || D.n_blosclz || D.n_snappy) ? (uint32_t *)P.grow(P.blosc.lzl, 2 * (D.n_sub + 1) * 4) : nullptr;
  if (D.n_zstd) {
    // k_blosc_finish reads raw / rle / literal-only zstd blocks where they lie (ZGPU_BLOSC_ALIAS=0: off)
    const char *ae = std::getenv("ZGPU_BLOSC_ALIAS");  // read per call (tests switch it)
    D.zs.knobs = zstd_knobs_from_env();
    zstd_bind(D.zs, D.n_sub, D.sub_slot, ZstdWants{!ae || std::atoi(ae) != 0, false, D.zs.knobs},
              [&](int k, uint64_t bytes) { return P.grow(P.blosc.zs[k], bytes); });
    D.zs.counters = P.zstd.zs.counters;
    D.zs.alias_count = P.d_counter + CTR_BLOSC_ALIASED;
    D.zs.max_nblk = P.zstd.zs.max_nblk;
    D.zs.ser_count = P.zstd.zs.ser_count;
    D.zs.launch_serial = P.zstd.zs.launch_serial;
    P.zstd_fork(D.zs, s);
  }
  // the layout (bases, inert tails past this execution's totals) is always computed on the device
  HIPCHK(launch_blosc_layout(info, ni, d_bases, caps, D, s));
  HIPCHK(launch_blosc_decode(P.d_items, P.d_status, ni, info, D, dst, P.L.slot_bytes, s));
}

// Enqueue the decode of an uploaded plan on stream s.
void plan_enqueue(zgpu_plan &P, uint8_t *out, hipStream_t s) {
  const uint32_t ni = (uint32_t)P.L.items.size();
  P.last_out = out;
  P.bz2.rounds = 0;
  HIPCHK(hipMemsetAsync(P.d_ctl, 0, P.ctl_bytes, s));
  if (!ni) return;
  P.zstd.zs.launch_serial = P.zstd.serial_off ? 0u : 1u;
  P.zstd.serial_skipped = P.zstd.serial_off;
  // stages rewrite each item's {src,len} in place; a chain with none reads the uploaded table as is
  const bool mutates = P.L.sharded || !P.L.stages.empty();
  ZgItem *items = mutates ? P.d_items : P.d_items_init;
  if (mutates)
    HIPCHK(hipMemcpyAsync(P.d_items, P.d_items_init, ni * sizeof(ZgItem), hipMemcpyDeviceToDevice, s));
  if (P.L.sharded) {
    HIPCHK(launch_shard_index(P.d_shards, (uint32_t)P.L.shards.size(), P.L.ispec, P.d_index, P.d_shard_status, 0, s));
    if (P.L.nested && !P.L.mids.empty()) {
      // middle shards: resolved through the outer index, their indexes decoded, then the leaves
      // resolve through them (a middle-shard error reaches every leaf of it via its status)
      const uint32_t nm = (uint32_t)P.L.mids.size();
      HIPCHK(hipMemcpyAsync(P.d_mids, P.d_mids_init, nm * sizeof(ZgItem), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemsetAsync(P.d_mid_status, 0, nm * 4, s));
      HIPCHK(launch_item_resolve(P.d_mids, P.d_mid_status, nm, P.d_shards, P.d_index, P.d_shard_status,
                                 P.L.ispec.n_inner, P.d_counter + CTR_SCRATCH, s));
      HIPCHK(launch_mid_shards(P.d_mids, P.d_mid_status, nm, P.d_mid_shards, P.d_shard_status2, s));
      HIPCHK(launch_shard_index(P.d_mid_shards, nm, P.L.ispec2, P.d_index2, P.d_shard_status2, 1, s));
      HIPCHK(launch_item_resolve(P.d_items, P.d_status, ni, P.d_mid_shards, P.d_index2, P.d_shard_status2,
                                 P.L.ispec2.n_inner, P.d_counter + CTR_ENC_BYTES, s));
    } else if (!P.L.nested) {
      HIPCHK(launch_item_resolve(P.d_items, P.d_status, ni, P.d_shards, P.d_index, P.d_shard_status, P.L.ispec.n_inner,
                                 P.d_counter, s));
    }
  }
  int crc_tail = 0;  // a trailing crc32c stage handed to the next gzip stage (launch_gzip places it)
  bool wrote_direct = false;  // a stage wrote whole items into the output (the scatter lists the rest)
  uint64_t len_hint = P.in_len_hint;  // of the current stage's input (a slot after a materialising stage)
  for (size_t si = 0; si < P.L.stages.size(); si++) {
    const Stage &st = P.L.stages[si];
    switch (st.kind) {
      case ST_ADLER32:
      case ST_FLETCHER32: {
        HIPCHK(launch_linsum_strip(st.kind == ST_ADLER32 ? CK_ADLER32 : CK_FLETCHER32, P.d_items, P.d_status, ni,
                                   st.at_start, P.validate ? 1 : 0, len_hint, P.ck_parts.p, s));  // sized in plan_upload
        break;
      }
      case ST_ZLIB:
        HIPCHK(launch_zlib_items(P.d_items, P.d_status, ni, P.d_pool[st.pool], P.L.slot_bytes, P.gzip.d_order, P.gzip.d_seg,
                                 s));
        break;
      case ST_BZ2:
        P.bz2.bz.blocks = P.d_counter + CTR_BZ2_BLOCKS;
        P.bz2.rounds += (ni + P.bz2.bz.round_items - 1) / P.bz2.bz.round_items;
        HIPCHK(launch_bz2(P.d_items, P.d_status, ni, P.d_pool[st.pool], P.L.slot_bytes, P.bz2.bz, s));
        break;
      case ST_CRC32C:
        if (!st.at_start && si + 1 < P.L.stages.size() && P.L.stages[si + 1].kind == ST_GZIP && P.gzip.d_seg) {
          crc_tail = P.validate ? 1 : 2;
          break;
        }
        HIPCHK(launch_crc32c_strip(P.d_items, P.d_status, ni, st.at_start, P.validate ? 1 : 0, s));
        break;
      case ST_GZIP: {
        GzDirect gd = P.L.gz;
        const bool direct = P.L.gz_direct && si + 1 == P.L.stages.size() && !P.L.no_scatter && out &&
                            ((uintptr_t)out & 15) == 0;
        gd.dout = direct ? out : nullptr;
        gd.geom = P.d_geom;
        // A/B (ZGPU_GZIP_CRC_FORK=1): the trailing crc32c checked on the plan's side stream beside the
        // one-wave kernel instead of by k_crc32c_strip ahead of it. It loses on C3 (18.11-18.18 ms against
        // 17.75-17.83 on one box, profiles/r06/r06cf_c3_gzip_crc_fork_ab.txt): the check's workgroups take
        // CU slots from the latency-bound decode
        GzCrcFork cf{};
        const char *fe = std::getenv("ZGPU_GZIP_CRC_FORK");
        const bool fork = crc_tail == 1 && fe && std::atoi(fe) != 0 && !(P.flags & ZGPU_ONE_STREAM);
        if (fork) {
          P.zstd_fork(P.zstd.zs, s);  // creates the plan's side stream and events (one compressor per chain)
        }
        if (fork && P.zstd.side.stream) {
          const size_t nb = (size_t)ni * (sizeof(ZgItem) + 8);
          uint8_t *scr = (uint8_t *)P.grow(P.gzip.crc, nb);
          cf.side = P.zstd.side.stream;
          cf.ev_fork = P.zstd.side.ev[0];
          cf.ev_join = P.zstd.side.ev[1];
          cf.snap_items = (ZgItem *)scr;
          cf.snap_status = (uint32_t *)(scr + (size_t)ni * sizeof(ZgItem));
          cf.bad = cf.snap_status + ni;
        }
        HIPCHK(launch_gzip(P.d_items, P.d_status, ni, P.d_pool[st.pool], P.L.slot_bytes, P.gzip.d_order, P.gzip.d_seg, s,
                           crc_tail, direct ? &gd : nullptr, cf.side ? &cf : nullptr));
        wrote_direct = wrote_direct || direct;
      }
        crc_tail = 0;
        break;
      case ST_ZSTD:
        P.zstd_fork(P.zstd.zs, s);
        P.zstd.zs.knobs = zstd_knobs_from_env();
        P.zstd.zs.lits_first = (P.flags & ZGPU_ZSTD_LITS_FIRST) && !P.zstd.zs.side ? 1u : 0u;
        HIPCHK(launch_zstd(P.d_items, P.d_status, ni, P.d_pool[st.pool], P.L.slot_bytes, P.zstd.zs, s));
        break;
      case ST_BLOSC:
        blosc_stage(P, st, out, s);
        break;
      case ST_UNSHUFFLE:
        HIPCHK(launch_unshuffle(P.d_items, P.d_status, ni, P.d_pool[st.pool], P.L.slot_bytes, st.elementsize, s));
        break;
    }
    if (!strips_only(st.kind)) len_hint = P.L.slot_bytes;
  }
  if (!P.L.no_scatter) {
    // A/B (ZGPU_SCATTER_LIST=1): after the gzip direct rows, the rows scatter over a device-built list
    // of the items still to write instead of the full grid whose written items' blocks exit at once;
    // it lost on C3 (18.22-18.33 vs 17.87-17.94 ms, profiles/r06/r06sl_c3_scatter_list_ab.txt)
    const char *le = std::getenv("ZGPU_SCATTER_LIST");
    uint32_t *live = nullptr;
    if (wrote_direct && le && std::atoi(le) != 0)
      live = (uint32_t *)P.grow(P.live_list, ((size_t)ni + 1) * 4);
    // both switches are read per launch (tests and A/B runs flip them in one process)
    const char *pe = std::getenv("ZGPU_TILED_PERSIST");
    const bool persist = P.L.tiled_p && (!pe || std::atoi(pe) != 0) && ((uintptr_t)out & 15) == 0;
    if (persist) {
      const char *ge = std::getenv("ZGPU_TILED_GRID");
      const uint32_t cap = ge ? (uint32_t)std::strtoul(ge, nullptr, 10) : 0;
      HIPCHK(launch_scatter_tiled_p(items, P.d_geom, P.d_status, P.d_origin, P.L.scatter, P.L.tiled_q, out, ni, cap, s));
      P.last_path = ZGPU_SCATTER_TILED_PERSISTENT;
    } else {
      HIPCHK(launch_scatter(items, P.d_geom, P.d_status, P.L.scatter, out, ni, P.L.scatter_mode, P.L.scatter_units, s, live));
      P.last_path = P.L.scatter_mode;
    }
  }
}

// InvalidBytesLengthError{len, expected_len} of descriptor d's first mismatching leaf item: the item's
// current {src,len} is the decoded representation the final stage rejected. A materialising stage
// that overflowed its slot leaves src on its input: the decoded length is then only known to exceed
// the expected one (len = UINT64_MAX).
static void size_detail(zgpu_plan &P, uint64_t d, const uint32_t *st, hipStream_t s) {
  const size_t ni = P.L.items.size();
  for (size_t i = 0; i < ni; i++) {
    if (P.L.items[i].desc != d || st[i] != ZGPU_DECODED_SIZE_MISMATCH) continue;
    const bool mutates = P.L.sharded || !P.L.stages.empty();
    ZgItem it{};
    HIPCHK(hipMemcpyAsync(&it, (mutates ? P.d_items : P.d_items_init) + i, sizeof(ZgItem), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    bool materialised = false, exact = true;
    for (const Stage &stg : P.L.stages)
      if (!strips_only(stg.kind)) materialised = true;
    if (materialised) {
      exact = false;
      for (int k = 0; k < P.L.n_pools; k++) {
        const uint64_t lo = (uint64_t)P.d_pool[k], hi = lo + ni * P.L.slot_bytes;
        if (it.src >= lo && it.src < hi) exact = true;
      }
    }
    size_detail().valid = 1;
    size_detail().desc = d;
    size_detail().len = exact ? it.len : UINT64_MAX;
    size_detail().expected = P.L.scatter.nelem * P.L.scatter.es;
    return;
  }
}

// Read back per-item statuses and reduce them to per-descriptor statuses. Returns the first
// non-zero descriptor status.
int plan_statuses(zgpu_plan &P, int32_t *status, hipStream_t s) {
  const size_t ni = P.L.items.size();
  HIPCHK(hipMemcpyAsync(P.h_ctl, P.d_ctl, P.ctl_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (((const uint64_t *)P.h_ctl)[CTR_BLOSC_OVF]) {
    // the input outgrew the cached blosc layout: nothing was decoded; re-run with a read-back layout
    P.blosc.caps_valid = false;
    plan_enqueue(P, P.last_out, s);
    HIPCHK(hipMemcpyAsync(P.h_ctl, P.d_ctl, P.ctl_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ((uint64_t *)P.h_ctl)[CTR_BLOSC_RERUN] = 1;
  }
  if (((const uint64_t *)P.h_ctl)[CTR_ZSTD_SERIAL]) {
    if (P.zstd.serial_skipped) {
      // this input has items for the serial zstd decoder, whose launch the plan skipped: re-run with it
      P.zstd.serial_off = false;
      plan_enqueue(P, P.last_out, s);
      HIPCHK(hipMemcpyAsync(P.h_ctl, P.d_ctl, P.ctl_bytes, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
    }
  } else if (((const uint64_t *)P.h_ctl)[CTR_ZSTD_PARALLEL]) {
    P.zstd.serial_off = true;  // no serial item: later executions do not launch the fallback
  }
  std::memcpy(P.last_counters, P.h_ctl, sizeof(P.last_counters));
  P.last_counters[CTR_ITEMS] = ni;
  P.last_counters[CTR_BZ2_ROUNDS] = P.bz2.rounds;
  for (int k = 0; k < CTR_N; k++) call_counters()[k] += P.last_counters[k];
  const uint32_t *st = (const uint32_t *)(P.h_ctl + 256);
  P.last_enc_bytes = P.last_counters[CTR_ENC_BYTES];
  std::vector<int32_t> ds(P.L.item_desc_status.begin(), P.L.item_desc_status.end());
  for (size_t i = 0; i < ni; i++) {
    const uint32_t d = P.L.items[i].desc;
    if (st[i] && ds[d] == 0) ds[d] = (int32_t)st[i];
  }
  int first = 0;
  uint64_t first_d = 0;
  for (uint64_t d = 0; d < P.n_desc; d++) {
    if (status) status[d] = ds[d];
    if (!first && ds[d]) {
      first = ds[d];
      first_d = d;
    }
  }
  if (first == ZGPU_DECODED_SIZE_MISMATCH && !size_detail().valid) size_detail(P, first_d, st, s);
  return first;
}

zgpu_plan *plan_new(zgpu_ctx *ctx, const std::shared_ptr<Chain> &chain, bool validate, uint32_t nd,
                    const zgpu_chunk_desc *descs, uint64_t n, const uint64_t *out_shape, uint32_t flags) {
  const bool checks = validate && !(flags & ZGPU_NO_VALIDATE);
  // the environment is read here, once per plan (tests and A/B runs flip the switches between plans)
  auto P = std::make_unique<zgpu_plan>(
      ctx, plan_layout(*chain, checks, nd, descs, n, out_shape, layout_knobs_from_env()));
  P->chain = chain;
  P->validate = checks;
  P->nd = nd;
  P->n_desc = n;
  P->flags = flags;
  P->out_shape.assign(out_shape, out_shape + nd);
  return P.release();
}

// hip_stream NULL: the context's stream, ordered after all work already queued on the legacy
// default stream (where torch's default stream and plain hipMemcpy/kernels land), so device buffers a
// caller produced there are complete before the decode reads or writes them.
hipStream_t pick_stream(Lane *L, void *s) {
  if (s) return (hipStream_t)s;
  if (!L->order_ev) HIPCHK(hipEventCreateWithFlags(&L->order_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(L->order_ev, nullptr));
  HIPCHK(hipStreamWaitEvent(L->stream, L->order_ev, 0));
  return L->stream;
}

// a plan's own stream (executes without a caller stream: an asynchronous execute and its later
// zgpu_plan_status must meet on one stream)
Lane *plan_lane(zgpu_plan &P) {
  if (!P.own.stream) HIPCHK(hipStreamCreateWithFlags(&P.own.stream, hipStreamNonBlocking));
  return &P.own;
}
