// The write path's host layout from C++ without a device: encode_layout (zarrs_amd/csrc/encode_layout.hpp)
// and the three size functions on one JSON case, printed as JSON for tests/test_encode_layout.py.
//   encode_layout_harness <case json>
// A case: {"codecs", "data_type", "fill" (hex bytes), "nd", "chunk_shape"}.
// Prints {"sizes": {"fixed", "chain_bound", "bound"}, "layout": {...}} or, for a refused chain,
// {"sizes": {...}, "err": <status>, "msg": "..."}; "ERR <status> <message>" if the chain does not parse.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/zgpu.h"
#include "../../zarrs_amd/csrc/encode_layout.hpp"

using namespace zgpu;

static const Json &need(const Json &j, const char *k) {
  const Json *v = j.get(k);
  if (!v) throw std::runtime_error(std::string("case lacks '") + k + "'");
  return *v;
}

typedef unsigned long long ull;

static void put_layout(const char *name, const EncodeLayout *L, uint32_t nd, const char *tail) {
  if (!L) {
    std::printf("\"%s\":null%s", name, tail);
    return;
  }
  std::printf("\"%s\":{\"path\":%u,\"es\":%u,\"shuffle\":%d,\"nelem\":%llu,\"data_bytes\":%llu,\"data_off\":%llu,\"stages\":[", name,
              (unsigned)L->path, L->chain->enc_es, L->shuffle ? 1 : 0, (ull)L->nelem, (ull)L->data_bytes, (ull)L->data_off);
  for (size_t i = 0; i < L->stages.size(); i++) {
    const EncodeStage &s = L->stages[i];
    std::printf("%s{\"kind\":%d,\"at_start\":%d,\"in\":%llu,\"out\":%llu,\"lo\":%llu,\"pool\":%d,\"level\":%d,\"zstd_checksum\":%d,"
                "\"zlib\":%d,\"zlib_bounded\":%d,\"blosc\":[%u,%u,%u,%llu]}",
                i ? "," : "", (int)s.kind, s.at_start, (ull)s.in_bound, (ull)s.out_bound, (ull)s.lo, s.pool, s.level,
                s.zstd_checksum ? 1 : 0, s.zlib ? 1 : 0, s.zlib_bounded ? 1 : 0, s.bl_comp, s.bl_shuffle, s.bl_typesize,
                (ull)s.bl_blocksize);
  }
  std::printf("],\"headroom\":%llu,\"pitch\":%llu,\"n_pools\":%d,\"fixed\":%d,\"size\":%llu,\"cps\":[", (ull)L->headroom,
              (ull)L->pitch, L->n_pools, L->fixed ? 1 : 0, (ull)L->size);
  for (uint32_t d = 0; d < nd && L->n_inner; d++) std::printf("%s%llu", d ? "," : "", (ull)L->cps[d]);
  std::printf("],\"n_inner\":%llu,\"inner_n\":%llu,\"index_at_start\":%d,\"index_big_endian\":%d,", (ull)L->n_inner,
              (ull)L->inner_n, L->index_at_start ? 1 : 0, L->index_big_endian ? 1 : 0);
  put_layout("inner", L->inner.get(), nd, ",");
  put_layout("index", L->index.get(), 1, ",");
  put_layout("native", L->native.get(), nd, ",");
  put_layout("packed", L->packed.get(), 1, ",");
  std::printf("\"packed_len\":%llu,\"upitch\":%llu,\"ppitch\":%llu,\"direct\":%d}%s", (ull)L->packed_len, (ull)L->upitch,
              (ull)L->ppitch, L->direct ? 1 : 0, tail);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  try {
    const Json c = Json::parse(argv[1]);
    uint8_t fill[16] = {0};
    const std::string &fh = need(c, "fill").as_str();
    for (size_t i = 0; i < fh.size() / 2 && i < 16; i++) {
      unsigned v = 0;
      std::sscanf(fh.c_str() + 2 * i, "%2x", &v);
      fill[i] = (uint8_t)v;
    }
    const auto chain = parse_chain(need(c, "codecs"), need(c, "data_type").as_str(), fill);
    const uint32_t nd = (uint32_t)need(c, "nd").as_int();
    uint64_t shape[ZGPU_MAX_DIMS] = {0}, n = 1;
    const Json &sj = need(c, "chunk_shape");
    if (nd == 0 || nd > ZGPU_MAX_DIMS || sj.arr.size() != nd) throw std::runtime_error("bad nd / chunk_shape");
    for (uint32_t d = 0; d < nd; d++) n *= shape[d] = (uint64_t)sj.arr[d].as_int();
    std::printf("{\"sizes\":{\"fixed\":%lld,\"chain_bound\":%lld,\"bound\":%lld},", (long long)chain_fixed_encoded_size(*chain, n),
                (long long)chain_encoded_bound(*chain, n), (long long)encoded_bound(*chain, nd, shape));
    try {
      const EncodeLayout L = encode_layout(*chain, nd, shape);
      put_layout("layout", &L, nd, "}\n");
    } catch (const ChainError &e) {
      std::string msg;
      for (char ch : e.msg) msg += (ch == '"' || ch == '\\') ? '\'' : ch;
      std::printf("\"err\":%d,\"msg\":\"%s\"}\n", e.status, msg.c_str());
    }
  } catch (const ChainError &e) {
    std::printf("ERR %d %s\n", e.status, e.msg.c_str());
  } catch (const std::exception &e) {
    std::printf("ERR %d %s\n", ZGPU_INVALID_ARGUMENT, e.what());
  }
  return 0;
}
