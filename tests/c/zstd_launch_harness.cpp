// The zstd decoder's host launch policy from C++ without a device: zstd_scratch_sizes and
// zstd_launch_policy (zarrs_amd/csrc/zstd_launch.hpp) on one JSON case, printed as JSON for
// tests/test_zstd_launch.py.
//   zstd_launch_harness <case json> [<case json> ...]
// A case: {"n_items", "slot", "cus", "knobs": {"xwin", "xpar", "xdense", "force_serial"}, "wants": {"alias",
// "latency"}, "caps": {"side", "alias", "lits_first", "ext", "lit_rec_wgs", "ser_list", "launch_serial"}}; a
// caps field left out (or "ext" / "lit_rec_wgs" given as -1) is what the sizes of the same case provide.
// Prints one line per case: {"sizes": {...}, "launch": {...}, "latency_possible": 0/1}. Needs only
// zstd_launch.cpp (the host sanitizer run compiles the two together) and a JSON reader of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../zarrs_amd/csrc/zstd_launch.hpp"

using namespace zgpu;

// the integer after "key": in a flat case object (every value a number or a nested object of numbers)
static long long field(const std::string &j, const char *obj, const char *key, long long absent) {
  size_t lo = 0, hi = j.size();
  if (obj) {
    lo = j.find(std::string("\"") + obj + "\"");
    if (lo == std::string::npos) return absent;
    lo = j.find('{', lo);
    hi = j.find('}', lo);
  }
  const size_t k = j.find(std::string("\"") + key + "\"", lo);
  if (k == std::string::npos || k >= hi) return absent;
  return std::strtoll(j.c_str() + j.find(':', k) + 1, nullptr, 10);
}

static const char *EXEC[] = {"LATENCY", "WINDOW", "WAVE_DENSE", "WAVE_WIDE"};
static const char *SERIAL[] = {"NONE", "PER_ITEM", "LISTED"};

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "env")) {  // the knobs as the environment gives them
    const ZstdKnobs K = zstd_knobs_from_env();
    std::printf("{\"xwin\":%d,\"xpar\":%d,\"xdense\":%d,\"force_serial\":%d}\n", K.xwin, K.xpar, K.xdense, K.force_serial);
    return 0;
  }
  for (int a = 1; a < argc; a++) {
    const std::string j = argv[a];
    const uint64_t n = (uint64_t)field(j, nullptr, "n_items", 0), slot = (uint64_t)field(j, nullptr, "slot", 0);
    const uint32_t cus = (uint32_t)field(j, nullptr, "cus", 0);
    ZstdKnobs K;
    K.xwin = (int)field(j, "knobs", "xwin", -1);
    K.xpar = field(j, "knobs", "xpar", 1) != 0;
    K.xdense = (int)field(j, "knobs", "xdense", -1);
    K.force_serial = field(j, "knobs", "force_serial", 0) != 0;
    const ZstdWants W{field(j, "wants", "alias", 0) != 0, field(j, "wants", "latency", 0) != 0, K};
    const ZstdScratchSizes S = zstd_scratch_sizes(n, slot, cus, W);
    ZstdCaps C;
    C.side = field(j, "caps", "side", 0) != 0;
    C.alias = field(j, "caps", "alias", S.alias != 0) != 0;
    C.lits_first = field(j, "caps", "lits_first", 0) != 0;
    const long long ext = field(j, "caps", "ext", -1), wgs = field(j, "caps", "lit_rec_wgs", -1);
    C.ext = ext < 0 ? S.ext != 0 : ext != 0;
    C.lit_rec_wgs = wgs < 0 ? S.lit_rec_wgs : (uint32_t)wgs;
    C.ser_list = field(j, "caps", "ser_list", 1) != 0;
    C.launch_serial = field(j, "caps", "launch_serial", 1) != 0;
    const ZstdLaunch L = zstd_launch_policy(n, slot, cus, C, K);
    std::printf("{\"sizes\":{\"blk_cap\":%u,\"lit_stride\":%llu,\"seq_cap\":%llu,\"lit_rec_wgs\":%u,\"blks\":%llu,"
                "\"norm\":%llu,\"nblk\":%llu,\"mode\":%llu,\"lit\":%llu,\"seq\":%llu,\"ser_list\":%llu,\"lit_rec\":%llu,"
                "\"alias\":%llu,\"ext\":%llu,\"ext_cnt\":%llu},",
                S.blk_cap, (unsigned long long)S.lit_stride, (unsigned long long)S.seq_cap, S.lit_rec_wgs,
                (unsigned long long)S.blks, (unsigned long long)S.norm, (unsigned long long)S.nblk,
                (unsigned long long)S.mode, (unsigned long long)S.lit, (unsigned long long)S.seq,
                (unsigned long long)S.ser_list, (unsigned long long)S.lit_rec, (unsigned long long)S.alias,
                (unsigned long long)S.ext, (unsigned long long)S.ext_cnt);
    std::printf("\"launch\":{\"grid\":%u,\"lgrid\":%u,\"bgrid\":%u,\"fork\":%d,\"lits_first\":%d,\"lit_direct\":%d,"
                "\"rec_slots\":%d,\"xseg\":%u,\"executor\":\"%s\",\"rounds\":%u,\"round_grid\":%u,\"persist_grid\":%u,"
                "\"serial\":\"%s\",\"serial_grid\":%u},\"latency_possible\":%d}\n",
                L.grid, L.lgrid, L.bgrid, L.fork, L.lits_first, L.lit_direct, L.rec_slots, L.xseg, EXEC[(uint32_t)L.executor],
                L.rounds, L.round_grid, L.persist_grid, SERIAL[(uint32_t)L.serial], L.serial_grid,
                zstd_latency_possible(n, slot, cus, K) ? 1 : 0);
  }
  return 0;
}
