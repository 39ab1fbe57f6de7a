// The cast_value element function on the host, without the library or a device: kernels/cast.hpp alone,
// for tests/test_cast_value_host.py (built with the undefined-behaviour and float-cast-overflow
// sanitizers, so an unchecked conversion aborts the run). Reads one case per line from standard input:
//   cast <source type> <target type> <rounding> <none|clamp|wrap> <elements as hex bytes, or ->
//        [<key hex>=<value hex> ...]      prints "OK <result hex bytes>" or "ERR <index of the first failure>"
//   infallible <source type> <target type> <none|clamp|wrap>     prints "0" or "1"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../zarrs_amd/csrc/kernels/cast.hpp"

using namespace zgpu;

static const char *TYPES[] = {"int8",   "int16",  "int32",   "int64",   "uint8",   "uint16",
                              "uint32", "uint64", "float32", "float64", "float16", "bfloat16"};
static const char *ROUNDINGS[] = {"nearest-even", "towards-zero", "towards-positive", "towards-negative", "nearest-away"};
static const char *OOR[] = {"none", "clamp", "wrap"};

template <size_t N>
static uint32_t index_of(const char *(&names)[N], const std::string &s) {
  for (uint32_t i = 0; i < N; i++)
    if (s == names[i]) return i;
  std::fprintf(stderr, "unknown name '%s'\n", s.c_str());
  std::exit(2);
}

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static uint64_t le_value(const std::vector<uint8_t> &b) {
  uint64_t v = 0;
  for (size_t i = 0; i < b.size() && i < 8; i++) v |= (uint64_t)b[i] << (8 * i);
  return v;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, s, t, r, o, hex, kv;
    in >> cmd;
    if (cmd == "infallible") {
      in >> s >> t >> o;
      std::printf("%d\n", cast_infallible(index_of(TYPES, s), index_of(TYPES, t), index_of(OOR, o)) ? 1 : 0);
      continue;
    }
    if (cmd != "cast") continue;
    in >> s >> t >> r >> o >> hex;
    const uint32_t cs = index_of(TYPES, s), ct = index_of(TYPES, t);
    CastMap map{};
    while (in >> kv && map.n < CAST_MAP_MAX) {
      const size_t eq = kv.find('=');
      map.key[map.n] = le_value(unhex(kv.substr(0, eq)));
      map.val[map.n] = le_value(unhex(kv.substr(eq + 1)));
      map.n++;
    }
    const std::vector<uint8_t> src = unhex(hex);
    const uint64_t n = src.size() / cast_type_size(cs);
    std::vector<uint8_t> dst(n * cast_type_size(ct) + 1);
    const uint64_t bad = cast_elements_host(cs, ct, src.data(), dst.data(), n, map, index_of(ROUNDINGS, r), index_of(OOR, o));
    if (bad != n) {
      std::printf("ERR %llu\n", (unsigned long long)bad);
      continue;
    }
    std::printf("OK ");
    for (uint64_t i = 0; i < n * cast_type_size(ct); i++) std::printf("%02x", dst[i]);
    std::printf("\n");
  }
  return 0;
}
