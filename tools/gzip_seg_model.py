"""CPU model of k_gzip's segmented symbol decode (kernels/inflate.hip, "segmented rounds"): the check of
its synchronisation logic against zlib, and the source of its sync statistics.

A Huffman block is decoded in rounds. In a round starting at the true bit position r0, lane l owns
the stream region [r0 + l*SEGB, r0 + (l+1)*SEGB) and decodes serially from OVL bits before it (lane 0
from r0). Its symbols starting inside its region are its records; `mask` marks which of the region's
first 64 bit positions start a symbol on its chain. Lane l is right when lane l-1 is, ended normally
(its exit = the first symbol start past its region), and that exit starts a symbol on lane l's chain;
lane l's records before the exit are dropped. The first wrong lane is re-decoded from its
predecessor's exit (at most MAXREP times a round); the round ends at the last right lane.

inflate_stream() also keeps the batch executor's accounting (ExecAcct: batches, pending bytes, where
each match's source lies relative to the ring and the flushed output), each block's table shapes under
build_table's allocation rule (table_shape) and each dynamic header's lane-parallel decode windows
(header_windows): what tests/deflate_streams.py's cases state their intent over. KERNEL holds the
kernel's segment constants (inflate_seg's defaults are older values its own test relies on).

Test infrastructure (tests/test_gzip_seg_model.py, tests/test_deflate_streams_model.py), not the
product path.
"""
from __future__ import annotations

import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163,
            195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
END, EOB, BAD, CAP, PAST = 0, 1, 2, 4, 5


class Bits:
    def __init__(self, data: bytes):
        self.v = int.from_bytes(data, "little")
        self.n = len(data) * 8

    def get(self, p: int, k: int) -> int:
        return (self.v >> p) & ((1 << k) - 1)


def table(lens):
    """{(length, reversed code): symbol} for an LSB-first bit reader (RFC 1951 3.2.2)."""
    mx = max(lens) if lens else 0
    cnt = [0] * (mx + 2)
    for ln in lens:
        if ln:
            cnt[ln] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1 if b > 1 else 0
        nxt[b] = code
    t = {}
    for s, ln in enumerate(lens):
        if ln:
            c = nxt[ln]
            nxt[ln] += 1
            t[(ln, int(format(c, "0%db" % ln)[::-1], 2))] = s
    return t, mx


def read_sym(B: Bits, p: int, t, mx):
    for ln in range(1, mx + 1):
        s = t.get((ln, B.get(p, ln)))
        if s is not None:
            return s, ln
    return None, 0


def symbol(B: Bits, p: int, lt, dt):
    """(kind, record, bits, out_len) of the symbol at p: kind 0 literal/match, EOB, BAD."""
    s, ln = read_sym(B, p, *lt)
    if s is None or s > 285:
        return BAD, 0, 0, 0
    if s < 256:
        return 0, s, ln, 1
    if s == 256:
        return EOB, 0, ln, 0
    i = s - 257
    q = p + ln
    length = LEN_BASE[i] + B.get(q, LEN_EXTRA[i])
    q += LEN_EXTRA[i]
    d, dl = read_sym(B, q, *dt)
    if d is None or d > 29:
        return BAD, 0, 0, 0
    q += dl
    dist = DIST_BASE[d] + B.get(q, DIST_EXTRA[d])
    q += DIST_EXTRA[d]
    return 0, (1 << 31) | (dist << 9) | length, q - p, length


def seg_decode(B, p, s_own, s_end, end_bits, lt, dt, cap):
    recs, mask = [], 0
    while p < s_end:
        if p >= end_bits:
            return PAST, p, recs, mask
        kind, rec, nb, _ = symbol(B, p, lt, dt)
        own = p >= s_own
        if own and p - s_own < 64:
            mask |= 1 << (p - s_own)
        if kind != 0:
            if not own:
                return PAST, p, recs, mask
            if kind == EOB:
                return EOB, p + nb, recs, mask
            return BAD, p, recs, mask
        if own:
            if len(recs) == cap:
                return CAP, p, recs, mask
            recs.append(rec)
        p += nb
    return END, p, recs, mask


def _eob_start(lane, lt):
    """Start bit of the end-of-block code a lane stopped at (its exit is the bit after it)."""
    ln = next(ln for (ln, _), s in lt[0].items() if s == 256)
    return lane["p"] - ln


def decode_block_seg(B, r0, end_bits, lt, dt, segb, ovl, cap, maxrep, stats, rounds_out=None):
    """Records of one Huffman block from r0 and the bit after its end-of-block code."""
    out = []
    while True:
        lanes = []
        for l in range(64):
            s_own = r0 + l * segb
            p = s_own - ovl if l else r0
            st, p, recs, mask = seg_decode(B, p, s_own, s_own + segb, end_bits, lt, dt, cap)
            lanes.append(dict(s_own=s_own, st=st, p=p, recs=recs, mask=mask, skip=0, ok=l == 0, rep=False))
        for rep in range(maxrep + 1):
            for l in range(1, 64):
                L, P = lanes[l], lanes[l - 1]
                if L["rep"]:
                    continue
                e, d = P["p"], P["p"] - L["s_own"]
                L["ok"] = P["st"] == END and 0 <= d < 64 and (L["mask"] >> d) & 1 == 1
                L["skip"] = bin(L["mask"] & ((1 << d) - 1)).count("1") if L["ok"] else 0
            j = next((l for l in range(64) if not all(lanes[k]["ok"] for k in range(l + 1))), 64)
            j = next((l for l in range(64) if not lanes[l]["ok"]), 64)
            if j == 64:
                break
            if lanes[j - 1]["st"] != END or rep >= maxrep:
                if lanes[j - 1]["st"] == END:
                    stats["maxrep_cuts"] = stats.get("maxrep_cuts", 0) + 1  # the round cut by MAXREP
                for l in range(j, 64):
                    lanes[l]["ok"] = False
                break
            e = lanes[j - 1]["p"]
            st, p, recs, mask = seg_decode(B, e, e, lanes[j]["s_own"] + segb, end_bits, lt, dt, cap)
            lanes[j].update(st=st, p=p, recs=recs, mask=mask, skip=0, ok=True, rep=True)
            stats["repairs"] += 1
        J = next((l for l in range(64) if not lanes[l]["ok"]), 64)
        stats["rounds"] += 1
        stats["valid_lanes"] += J
        rnd = []
        for l in range(J):
            rnd.extend(lanes[l]["recs"][lanes[l]["skip"]:])
        out.extend(rnd)
        if rounds_out is not None:
            rounds_out.append(rnd)
        last = lanes[J - 1]
        if last["st"] == CAP:
            stats["cap_hits"] = stats.get("cap_hits", 0) + 1  # a lane region filled its SEGCAP records
        if last["st"] == EOB:
            # where the end-of-block code started: in the region of lane J-1 (off bits past its s_own;
            # to_end bits before its region's end, inside the next lane's overlap when <= ovl)
            q = _eob_start(last, lt)
            stats.setdefault("eob", []).append(dict(lane=J - 1, off=q - last["s_own"], repaired=last["rep"],
                                                    to_end=last["s_own"] + segb - q))
            return out, last["p"]
        if last["st"] in (END, CAP):
            r0 = last["p"]
            continue
        raise ValueError("corrupt stream (status %d)" % last["st"])


def inflate_seg(gz: bytes, segb=512, ovl=256, cap=64, maxrep=8, stats=None):
    """gzip member -> decoded bytes through the segmented decode (stored blocks copied directly)."""
    stats = stats if stats is not None else {}
    for k in ("rounds", "valid_lanes", "repairs", "blocks"):
        stats.setdefault(k, 0)
    assert gz[:3] == b"\x1f\x8b\x08"
    flg, hp = gz[3], 10
    if flg & 4:
        hp += 2 + int.from_bytes(gz[hp:hp + 2], "little")
    for f in (8, 16):
        if flg & f:
            hp = gz.index(b"\0", hp) + 1
    if flg & 2:
        hp += 2
    return inflate_stream(gz, hp, 8, segb, ovl, cap, maxrep, stats)


# The kernel's constants (kernels/inflate.hip): the segment decode's and the batch executor's.
KERNEL = dict(segb=512, ovl=384, cap=96, maxrep=8)
RING, BATCH_CAP, FLUSH_MIN, BATCH_SYMS = 1024, 480, 256, 64
# BATCH_CAP was RING / 2: up to RING bytes were then unflushed in a batch (B + f), and from RING - 30 on
# the executor read stale bytes (tests/deflate_streams.py's executor_ring family reaches that state
# under this value and must not under the kernel's)
BATCH_CAP_RING_HALF = 512


def table_shape(lens, root):
    """(longest code, second-level table entries) of a code set under the kernel's allocation rule
    (build_table): every root prefix of codes longer than the root gets 2^(its longest code - root)."""
    t, mx = table(lens)
    sub = {}
    for (ln, rc), _ in t.items():
        if ln > root:
            c = int(format(rc, "0%db" % ln)[::-1], 2)  # MSB-first code
            pre = c >> (ln - root)
            sub[pre] = max(sub.get(pre, 0), ln - root)
    return mx, sum(1 << b for b in sub.values())


def header_windows(syms, total):
    """The lane-parallel header decode's windows over a dynamic header's code-length symbols
    [(symbol, bits, lengths it writes)]: a window takes the symbols that start within its first 63
    bits, at most 32 of them, up to the header's last length. Per window: `take` (the symbols taken),
    `starts` (symbol starts within its 63 bits), `first` (index of its first length) and `last_end`
    (the window bit at which its last taken symbol ends: past 63 when that symbol reaches out of it)."""
    wins, i, n = [], 0, 0
    while n < total and i < len(syms):
        off, take, starts, j, first, last_end = 0, [], 0, i, n, 0
        while j < len(syms) and off < 63:
            starts += 1
            if len(take) < 32 and n < total:
                take.append(syms[j][0])
                n += syms[j][2]
                i = j + 1
                last_end = off + syms[j][1]
            off += syms[j][1]
            j += 1
        wins.append(dict(take=take, starts=starts, first=first, last_end=last_end))
    return wins


class ExecAcct:
    """The batch executor's accounting (exec_batch and its callers): a round's records go in batches of
    at most BATCH_SYMS symbols, taken while the batch holds fewer than batch_cap bytes; the ring is
    flushed once FLUSH_MIN bytes are pending; a stored block flushes everything. Per batch: B (its
    bytes), f (bytes pending at its start), and for each match where its source lies: the source start
    in the ring or older (`start_in_ring`: what the kernel's per-match test sees), and its last source
    byte flushed or not (`last_flushed`)."""

    def __init__(self, batch_cap=BATCH_CAP):
        self.pos = self.flushed = 0
        self.batches = []
        self.batch_cap = batch_cap

    def stored(self, n):
        self.pos += n
        self.flushed = self.pos

    def round(self, recs):
        g = 0
        while g < len(recs):
            b, k = 0, g
            while k < len(recs) and k - g < BATCH_SYMS and b < self.batch_cap:
                b += (recs[k] & 511) if recs[k] >> 31 else 1
                k += 1
            end, q, ms = self.pos + b, self.pos, []
            for r in recs[g:k]:
                if r >> 31:
                    dist, ln = (r >> 9) & 0xFFFF, r & 511
                    src = q - dist
                    ms.append(dict(len=ln, dist=dist, src=src, start_in_ring=src + RING >= end,
                                   last_flushed=src + min(ln, dist) - 1 < self.flushed,
                                   last=src + min(ln, dist) - 1))
                    q += ln
                else:
                    q += 1
            self.batches.append(dict(B=b, f=self.pos - self.flushed, pos=self.pos, flushed=self.flushed,
                                     syms=k - g, matches=ms))
            self.pos = end
            if self.pos - self.flushed >= FLUSH_MIN:
                self.flushed = self.pos
            g = k


def inflate_stream(data: bytes, start: int, trailer: int, segb=512, ovl=256, cap=64, maxrep=8, stats=None,
                   batch_cap=BATCH_CAP):
    """The DEFLATE stream at byte `start` of `data` (`trailer` bytes follow it) -> decoded bytes through
    the segmented decode, with the executor's accounting in stats["batches"], each Huffman block's
    table shapes in stats["tables"] and each dynamic header's windows in stats["hdr"]."""
    stats = stats if stats is not None else {}
    for k in ("rounds", "valid_lanes", "repairs", "blocks", "maxrep_cuts", "cap_hits"):
        stats.setdefault(k, 0)
    acct = ExecAcct(batch_cap)
    stats["batches"] = acct.batches
    gz, hp = data, start
    B = Bits(gz)
    end_bits = (len(gz) - trailer) * 8
    p, out, last = hp * 8, bytearray(), False
    while not last:
        last, typ = B.get(p, 1), B.get(p + 1, 2)
        p += 3
        stats["blocks"] += 1
        if typ == 0:
            p = (p + 7) & ~7
            n = B.get(p, 16)
            p += 32
            out += gz[p // 8:p // 8 + n]
            p += 8 * n
            acct.stored(n)
            continue
        if typ == 1:
            lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
            dl = [5] * 30
        else:
            hlit, hdist, hclen = B.get(p, 5) + 257, B.get(p + 5, 5) + 1, B.get(p + 10, 4) + 4
            p += 14
            cl = [0] * 19
            for i in range(hclen):
                cl[CLEN_ORDER[i]] = B.get(p, 3)
                p += 3
            ct = table(cl)
            ll, syms = [], []
            while len(ll) < hlit + hdist:
                s, n = read_sym(B, p, *ct)
                p += n
                k = len(ll)
                if s < 16:
                    ll.append(s)
                elif s == 16:
                    ll += [ll[-1]] * (3 + B.get(p, 2))
                    p += 2
                    n += 2
                elif s == 17:
                    ll += [0] * (3 + B.get(p, 3))
                    p += 3
                    n += 3
                else:
                    ll += [0] * (11 + B.get(p, 7))
                    p += 7
                    n += 7
                syms.append((s, n, len(ll) - k))
            assert len(ll) == hlit + hdist, "a run past the header's last length"
            stats.setdefault("hdr", []).append(dict(hlit=hlit, hdist=hdist, hclen=hclen, syms=syms, clmax=ct[1],
                                                    windows=header_windows(syms, hlit + hdist)))
            lens, dl = ll[:hlit], ll[hlit:]
        stats.setdefault("tables", []).append(dict(zip(("lmax", "lsub", "dmax", "dsub"),
                                                       table_shape(lens, 9) + table_shape(dl, 8))))
        rounds = []
        recs, p = decode_block_seg(B, p, end_bits, table(lens), table(dl), segb, ovl, cap, maxrep, stats, rounds)
        for rnd in rounds:
            acct.round(rnd)
        for r in recs:  # LZ77
            if r >> 31:
                dist, ln = (r >> 9) & 0xFFFF, r & 511
                for _ in range(ln):
                    out.append(out[-dist])
            else:
                out.append(r)
    return bytes(out)


if __name__ == "__main__":
    import numpy as np
    rng = np.random.default_rng(7)
    x = np.arange(32, dtype=np.float32)
    for lvl in (1, 6, 9):
        a = np.rint(256 * (np.sin(0.05 * x)[:, None, None] + np.cos(0.03 * x)[None, :, None]
                           + 0.5 * np.sin(0.07 * x)[None, None, :]) + rng.standard_normal((32, 32, 32))) / 256
        raw = a.astype(np.float32).tobytes()
        co = zlib.compressobj(lvl, zlib.DEFLATED, 31)
        gz = co.compress(raw) + co.flush()
        st = {}
        assert inflate_seg(gz, stats=st) == raw
        print(f"level {lvl}: {len(gz)} B, {st['blocks']} blocks, {st['rounds']} rounds, "
              f"{st['valid_lanes'] / st['rounds']:.1f} valid lanes/round, {st['repairs']} repairs")
