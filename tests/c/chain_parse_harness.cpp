// The chain model from C++ without a device: parse_chain (zarrs_amd/csrc/chain.hpp) on one codecs
// list, printed as one line for tests/test_chain_value_parse.py.
//   chain_parse_harness <codecs json> <data type> <fill value as hex bytes> <elements per chunk>
// prints "OK a2b=<kind> enc_type=<type> enc_fill=<hex> size=<fixed size> bound=<bound> value=<0|1> a2a=<n>
// inner_enc_type=<type|->" or "ERR <status> <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/zgpu.h"
#include "../../zarrs_amd/csrc/chain.hpp"

using namespace zgpu;

static const char *kind_name(CodecKind k) {
  switch (k) {
    case CodecKind::Bytes: return "bytes";
    case CodecKind::Sharding: return "sharding";
    case CodecKind::PackBits: return "packbits";
    default: return "other";
  }
}

static std::string hex(const uint8_t *p, uint32_t n) {
  std::string s;
  char b[3];
  for (uint32_t i = 0; i < n; i++) {
    std::snprintf(b, sizeof b, "%02x", p[i]);
    s += b;
  }
  return s;
}

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  uint8_t fill[16] = {0};
  const size_t nh = std::strlen(argv[3]) / 2;
  for (size_t i = 0; i < nh && i < 16; i++) {
    unsigned v = 0;
    std::sscanf(argv[3] + 2 * i, "%2x", &v);
    fill[i] = (uint8_t)v;
  }
  const uint64_t nelem = std::strtoull(argv[4], nullptr, 10);
  try {
    const Json j = Json::parse(argv[1]);
    const auto c = parse_chain(j, argv[2], fill);
    const Chain *leaf = c.get();
    while (leaf->a2b.kind == CodecKind::Sharding) leaf = leaf->a2b.inner.get();
    std::printf("OK a2b=%s enc_type=%s enc_fill=%s size=%lld bound=%lld value=%d a2a=%zu inner_enc_type=%s", kind_name(c->a2b.kind),
                c->enc_data_type.c_str(), hex(c->enc_fill, c->enc_es).c_str(), (long long)chain_fixed_encoded_size(*c, nelem),
                (long long)chain_encoded_bound(*c, nelem), chain_has_value_codec(*c) ? 1 : 0, c->a2a.size(),
                leaf == c.get() ? "-" : leaf->enc_data_type.c_str());
    if (c->a2b.kind == CodecKind::PackBits)
      std::printf(" bits=%u..%u comp=%u ncomp=%u signed=%d padding=%d", c->a2b.pb_first, c->a2b.pb_last, c->a2b.pb_comp_bits,
                  c->a2b.pb_ncomp, c->a2b.pb_signed ? 1 : 0, c->a2b.pb_padding);
    std::printf("\n");
  } catch (const ChainError &e) {
    std::printf("ERR %d %s\n", e.status, e.msg.c_str());
  } catch (const std::exception &e) {
    std::printf("ERR %d %s\n", ZGPU_INVALID_ARGUMENT, e.what());
  }
  return 0;
}
