"""The zstd decoder's host launch policy as DESIGN.md states it ("The launch policy in one table"),
written from those rules and not from zstd_launch.cpp: scratch sizes and every launch decision of a batch
of n_items slots of `slot` bytes on a device of `cus` compute units. tests/test_zstd_launch.py holds the
library to it."""
from math import ceil, log2

import zstd_frames as Z

MIB = 1 << 20
ZPAR_MAX_BYTES = 128 * MIB   # latency mode: decoded bytes per batch
ZEXT_ROUNDS = 24
ZBLK_BYTES = 160             # one block record
ZNORM_BYTES = 3 * 64 * 2     # three tables of 64 int16 counts per block record
LIT_GRID_PER_CU = 4          # k_zstd_lits workgroups per CU
LIT_THREADS, REC_SLOT = 256, 1024 + 64
BLK_WPE = 6                  # k_zstd_blocks waves per SIMD
XSEG_WIN, XSEG = 8, 12
XWIN_MAX_WPC, XDENSE_WPC = 4, 64
T = 1024                     # the window executors' sequence table
KNOBS = {"xwin": -1, "xpar": 1, "xdense": -1, "force_serial": 0}


def window_executors(n, cus, knobs):
    return knobs["xwin"] != 0 if knobs["xwin"] >= 0 else 3 * n < XWIN_MAX_WPC * cus


def latency_possible(n, slot, cus, knobs):
    return bool(window_executors(n, cus, knobs) and knobs["xpar"] and n * slot <= ZPAR_MAX_BYTES)


def rounds(slot):
    blk_cap = Z.layout(slot)[0]
    hops = blk_cap + 2 * (slot // Z.WSPAN) + slot // (3 * T) + 1
    return min(ceil(log2(hops)) + 1, ZEXT_ROUNDS)


def sizes(n, slot, cus, wants, knobs):
    blk_cap, lit_stride, seq_cap = Z.layout(slot)
    lat = wants["latency"] and latency_possible(n, slot, cus, knobs)
    return {"blk_cap": blk_cap, "lit_stride": lit_stride, "seq_cap": seq_cap, "lit_rec_wgs": cus * LIT_GRID_PER_CU,
            "blks": n * blk_cap * ZBLK_BYTES, "norm": n * blk_cap * ZNORM_BYTES, "nblk": 4 * n, "mode": 4 * n,
            "lit": n * lit_stride, "seq": n * seq_cap * 12, "ser_list": 4 * n,
            "lit_rec": cus * LIT_GRID_PER_CU * LIT_THREADS * REC_SLOT, "alias": n * 3 * 2 * 8 if wants["alias"] else 0,
            "ext": 8 * n * slot if lat else 0, "ext_cnt": 8 * ZEXT_ROUNDS if lat else 0}


def launch(n, slot, cus, caps, knobs):
    recs = n * Z.layout(slot)[0]
    L = {"grid": min(recs, cus * 16), "lgrid": min(recs, cus * LIT_GRID_PER_CU),
         "bgrid": min(recs, max(cus * 16, cus * 4 * BLK_WPE))}
    L["fork"] = int(caps["side"])
    L["lits_first"] = int(caps["lits_first"] and not L["fork"])
    L["lit_direct"] = int(not L["fork"] and not caps["alias"] and not L["lits_first"])
    L["rec_slots"] = int(L["lgrid"] <= caps["lit_rec_wgs"])
    win = window_executors(n, cus, knobs)
    L["xseg"] = XSEG_WIN if win else XSEG
    if win:
        L["executor"] = "LATENCY" if caps["ext"] and latency_possible(n, slot, cus, knobs) else "WINDOW"
    else:
        dense = knobs["xdense"] != 0 if knobs["xdense"] >= 0 else n * XSEG >= XDENSE_WPC * cus
        L["executor"] = "WAVE_DENSE" if dense else "WAVE_WIDE"
    lat = L["executor"] == "LATENCY"
    L["rounds"] = rounds(slot) if lat else 0
    L["round_grid"] = min((n * slot // 4 + 255) // 256, cus * 16) if lat else 0
    L["persist_grid"] = cus if lat else 0
    L["serial"] = "PER_ITEM" if not caps["ser_list"] else "LISTED" if caps["launch_serial"] else "NONE"
    L["serial_grid"] = {"PER_ITEM": n, "LISTED": min(n, 4 * cus), "NONE": 0}[L["serial"]]
    return L
