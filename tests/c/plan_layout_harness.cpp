// The fused plan's host layout from C++ without a device: plan_layout / stages_only_layout
// (zarrs_amd/csrc/plan_layout.hpp) on one JSON case, printed as JSON for tests/test_plan_layout.py.
//   plan_layout_harness <case json>
// A layout case: {"codecs", "data_type", "fill" (hex bytes), "nd", "out_shape", "validate", "knobs":
// {"unshuffle_wide", "blosc_no_direct", "gzip_direct", "blosc_no_partial"}, "descs": [{"chunk_shape",
// "sel_start", "sel_shape", "out_start", "present"}]}. Present chunk i gets the made-up encoded bytes
// {0x10000 * (i + 1), 1000 + i}, which nothing dereferences. A stages-only case: {"stages_only": {"kind",
// "at_start", "elementsize", "slot_bytes", "items": [[src, len], ...]}}.
// Prints the PlanLayout as one JSON object, or "ERR <status> <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zgpu.h"
#include "../../zarrs_amd/csrc/plan_layout.hpp"

using namespace zgpu;

static const Json &need(const Json &j, const char *k) {
  const Json *v = j.get(k);
  if (!v) throw std::runtime_error(std::string("case lacks '") + k + "'");
  return *v;
}

static void fill_u64(const Json &a, uint64_t *out) {
  for (size_t i = 0; i < a.arr.size() && i < ZGPU_MAX_DIMS; i++) out[i] = (uint64_t)a.arr[i].as_int();
}

template <class T>
static void put_list(const char *name, const T *p, size_t n, const char *tail = ",") {
  std::printf("\"%s\":[", name);
  for (size_t i = 0; i < n; i++) std::printf("%s%llu", i ? "," : "", (unsigned long long)p[i]);
  std::printf("]%s", tail);
}

static void put_items(const char *name, const std::vector<ZgItem> &v) {
  std::printf("\"%s\":[", name);
  for (size_t i = 0; i < v.size(); i++)
    std::printf("%s[%llu,%llu,%u,%u,%u,%u]", i ? "," : "", (unsigned long long)v[i].src, (unsigned long long)v[i].len,
                v[i].desc, v[i].flags, v[i].shard, v[i].inner);
  std::printf("],");
}

static void put_ispec(const char *name, const ZgIndexSpec &S) {
  std::printf("\"%s\":{\"n_inner\":%llu,\"index_bytes\":%llu,\"at_start\":%u,\"big_endian\":%u,\"n_crc\":%u,", name,
              (unsigned long long)S.n_inner, (unsigned long long)S.index_bytes, S.at_start, S.big_endian, S.n_crc);
  put_list("crc_at_start", S.crc_at_start, 4);
  std::printf("\"verify\":%u},", S.verify);
}

static void put_layout(const PlanLayout &L) {
  const uint32_t nd = L.scatter.nd;
  std::printf("{");
  put_items("items", L.items);
  put_list("geom", L.geom.data(), L.geom.size());
  put_list("item_desc_status", L.item_desc_status.data(), L.item_desc_status.size());
  std::printf("\"shards\":[");
  for (size_t i = 0; i < L.shards.size(); i++)
    std::printf("%s[%llu,%llu]", i ? "," : "", (unsigned long long)L.shards[i].ptr, (unsigned long long)L.shards[i].len);
  std::printf("],");
  put_items("mids", L.mids);
  put_ispec("ispec", L.ispec);
  put_ispec("ispec2", L.ispec2);
  std::printf("\"stages\":[");
  for (size_t i = 0; i < L.stages.size(); i++)
    std::printf("%s[%d,%d,%u,%d]", i ? "," : "", (int)L.stages[i].kind, L.stages[i].at_start, L.stages[i].elementsize,
                L.stages[i].pool);
  std::printf("],\"slot_bytes\":%llu,\"n_pools\":%d,", (unsigned long long)L.slot_bytes, L.n_pools);
  const ZgScatter &S = L.scatter;
  std::printf("\"scatter\":{\"nd\":%u,\"es\":%u,\"comp\":%u,\"swap\":%u,\"shuffle\":%u,\"tile_a\":%u,\"tile_b\":%u,\"pad0\":%u,",
              S.nd, S.es, S.comp, S.swap, S.shuffle, S.tile_a, S.tile_b, S.pad0);
  put_list("chunk_shape", S.chunk_shape, nd);
  put_list("enc_stride", S.enc_stride, nd);
  put_list("out_stride", S.out_stride, nd);
  put_list("fill", S.fill, 16);
  std::printf("\"nelem\":%llu},", (unsigned long long)S.nelem);
  std::printf("\"scatter_mode\":%u,\"scatter_units\":%llu,\"tiled_p\":%d,\"tiled_upi\":%u,", L.scatter_mode,
              (unsigned long long)L.scatter_units, L.tiled_p ? 1 : 0, L.tiled_q.upi);
  put_list("origin", L.origin.data(), L.origin.size());
  std::printf("\"first_path\":%u,\"sharded\":%d,\"nested\":%d,\"leaf_es\":%u,\"alg_bytes_static\":%llu,", L.first_path,
              L.sharded ? 1 : 0, L.nested ? 1 : 0, L.leaf ? L.leaf->es : 0, (unsigned long long)L.alg_bytes_static);
  std::printf("\"bl_direct\":%d,\"gz_direct\":%d,\"gz\":{\"want\":%llu,\"nd\":%u,\"lbs\":%u,", L.bl_direct ? 1 : 0,
              L.gz_direct ? 1 : 0, (unsigned long long)L.gz.want, L.gz.nd, L.gz.lbs);
  put_list("cshape", L.gz.cshape, 4);
  put_list("ostr", L.gz.ostr, 4, "},");
  // UINT64_MAX ("to the end") does not survive every JSON reader: as -1
  std::printf("\"bl_need\":[");
  for (size_t i = 0; i < L.bl_need.size(); i++)
    std::printf("%s%lld", i ? "," : "", L.bl_need[i] == UINT64_MAX ? -1ll : (long long)L.bl_need[i]);
  std::printf("],\"no_scatter\":%d}\n", L.no_scatter ? 1 : 0);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  try {
    const Json c = Json::parse(argv[1]);
    if (const Json *so = c.get("stages_only")) {
      std::vector<ZgItem> items;
      for (const Json &it : need(*so, "items").arr) {
        ZgItem z{};
        z.src = (uint64_t)it.arr.at(0).as_int();
        z.len = (uint64_t)it.arr.at(1).as_int();
        items.push_back(z);
      }
      Stage st{};
      st.kind = (StageKind)need(*so, "kind").as_int();
      st.at_start = (int)need(*so, "at_start").as_int();
      st.elementsize = (uint32_t)need(*so, "elementsize").as_int();
      put_layout(stages_only_layout(std::move(items), st, (uint64_t)need(*so, "slot_bytes").as_int()));
      return 0;
    }
    uint8_t fill[16] = {0};
    const std::string &fh = need(c, "fill").as_str();
    for (size_t i = 0; i < fh.size() / 2 && i < 16; i++) {
      unsigned v = 0;
      std::sscanf(fh.c_str() + 2 * i, "%2x", &v);
      fill[i] = (uint8_t)v;
    }
    const auto chain = parse_chain(need(c, "codecs"), need(c, "data_type").as_str(), fill);
    const uint32_t nd = (uint32_t)need(c, "nd").as_int();
    uint64_t out_shape[ZGPU_MAX_DIMS] = {0};
    fill_u64(need(c, "out_shape"), out_shape);
    const Json &kj = need(c, "knobs");
    LayoutKnobs K;
    K.unshuffle_wide = (uint32_t)need(kj, "unshuffle_wide").as_int();
    K.blosc_no_direct = need(kj, "blosc_no_direct").b;
    K.gzip_direct = need(kj, "gzip_direct").b;
    K.blosc_no_partial = need(kj, "blosc_no_partial").b;
    std::vector<zgpu_chunk_desc> descs;
    for (const Json &dj : need(c, "descs").arr) {
      zgpu_chunk_desc D;
      std::memset(&D, 0, sizeof D);
      const size_t i = descs.size();
      if (need(dj, "present").b) {
        D.enc = (const void *)(uintptr_t)(0x10000ull * (i + 1));
        D.enc_len = 1000 + i;
      }
      fill_u64(need(dj, "chunk_shape"), D.chunk_shape);
      fill_u64(need(dj, "sel_start"), D.sel_start);
      fill_u64(need(dj, "sel_shape"), D.sel_shape);
      fill_u64(need(dj, "out_start"), D.out_start);
      descs.push_back(D);
    }
    put_layout(plan_layout(*chain, need(c, "validate").b, nd, descs.data(), descs.size(), out_shape, K));
  } catch (const ChainError &e) {
    std::printf("ERR %d %s\n", e.status, e.msg.c_str());
  } catch (const std::exception &e) {
    std::printf("ERR %d %s\n", ZGPU_INVALID_ARGUMENT, e.what());
  }
  return 0;
}
