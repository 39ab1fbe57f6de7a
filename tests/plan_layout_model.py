"""A numpy model of the fused plan's host layout (zarrs_amd/csrc/plan_layout.hpp), written from zarrs'
rules and DESIGN.md rather than from the C++: element by element for the work items, and from numpy's own
strides for the scatter geometry. tests/test_plan_layout.py holds the library to it.

A case is the dictionary tests/c/plan_layout_harness.cpp reads: codecs, data_type, fill, nd, out_shape,
validate, knobs, descs (chunk_shape, sel_start, sel_shape, out_start, present). The harness gives present
chunk i the encoded bytes {0x10000 * (i + 1), 1000 + i}.

The rules:
 * a plain chunk is one work item with the descriptor's own selection; a descriptor of a sharded array
   gives one item per leaf chunk its selection meets, found here by walking every selected element
   through the transposes before sharding_indexed into the shard's encoded frame (codec_chain.rs:557-646)
   and grouping the elements by the leaf they fall in (sharding.rs:107-154);
 * items are ordered by descriptor, then by middle shard (nested sharding) in C order of the shard's
   grid of middle shards, then by leaf in C order of its grid;
 * a descriptor that is wrong by itself (selection past its chunk or the output, another chunk shape
   than the batch's, a shard its subchunks do not divide) gets INVALID_ARGUMENT and no items, a shard of
   another subchunk count than the batch's first UNSUPPORTED; a selection without elements gives no
   items, except that a whole chunk of zero extent still runs its checks.
"""
import itertools

import numpy as np

INVALID_ARGUMENT, UNSUPPORTED = 10, 6
FILL, PARTIAL, SHARDED = 1, 2, 4
ROWS, TILED, GENERIC, TILED_PERSISTENT = 0, 1, 2, 3
MAXD = 8
ST = {"crc32c": 0, "gzip": 1, "zstd": 2, "numcodecs.shuffle": 3, "blosc": 4, "numcodecs.adler32": 5,
      "numcodecs.fletcher32": 6, "numcodecs.zlib": 7, "numcodecs.bz2": 8}
CHECKSUMS = ("crc32c", "numcodecs.adler32", "numcodecs.fletcher32")
VALUE_CODECS = ("numcodecs.fixedscaleoffset", "bitround", "numcodecs.bitround", "packbits")
ES = {"uint8": 1, "int8": 1, "uint16": 2, "int16": 2, "float32": 4, "int32": 4, "uint32": 4, "float64": 8,
      "uint64": 8, "complex128": 16}
COMP = dict(ES, complex128=8)
KNOBS = {"unshuffle_wide": 0, "blosc_no_direct": False, "gzip_direct": True, "blosc_no_partial": False}
PRIMES = (2, 3, 5, 7, 11, 13, 17, 19)


class LayoutError(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def split(codecs):
    """(transpose orders, the array->bytes codec, bytes->bytes codecs) of a codecs list."""
    names = [c["name"] for c in codecs]
    k = next(i for i, n in enumerate(names) if n in ("bytes", "sharding_indexed", "packbits"))
    return [c["configuration"]["order"] for c in codecs[:k] if c["name"] == "transpose"], codecs[k], codecs[k + 1:]


def has_value_codec(codecs):
    for c in codecs:
        if c["name"] in VALUE_CODECS:
            return True
        if c["name"] == "sharding_indexed" and has_value_codec(c["configuration"]["codecs"]):
            return True
    return False


def through(a, orders, lead=0):
    """a as the codecs after the transposes see it; lead: leading axes that stay (np.indices' first)."""
    for o in orders:
        a = a.transpose(list(range(lead)) + [lead + k for k in o])
    return a


def axes_of(orders, nd):
    """m: encoded axis a is decoded axis m[a], read off the shape of a transposed array of distinct extents."""
    shape = through(np.broadcast_to(np.uint8(0), PRIMES[:nd]), orders).shape
    return [PRIMES.index(s) for s in shape]


def levels(case):
    """The chain's levels, with the errors of a chain the fused plan does not take."""
    nd, codecs = case["nd"], case["codecs"]
    if has_value_codec(codecs):
        raise LayoutError(UNSUPPORTED, "value codec or packbits")
    orders, a2b, b2b = split(codecs)
    V = {"outer": [], "sub": None, "mid": None, "index": [], "leaf_codecs": codecs}
    if a2b["name"] == "sharding_indexed":
        if any(len(o) != nd for o in orders):
            raise LayoutError(INVALID_ARGUMENT, "transpose rank")
        if b2b:
            raise LayoutError(UNSUPPORTED, "bytes->bytes after sharding_indexed")
        cfg = a2b["configuration"]
        if len(cfg["chunk_shape"]) != nd:
            raise LayoutError(INVALID_ARGUMENT, "chunk_shape rank")
        V.update(outer=orders, sub=list(cfg["chunk_shape"]), index=[cfg], leaf_codecs=cfg["codecs"])
        o2, a2, b2 = split(cfg["codecs"])
        if a2["name"] == "sharding_indexed":
            if o2 or b2 or len(cfg["codecs"]) != 1:
                raise LayoutError(UNSUPPORTED, "codecs around a nested sharding_indexed")
            c2 = a2["configuration"]
            if split(c2["codecs"])[1]["name"] == "sharding_indexed":
                raise LayoutError(UNSUPPORTED, "three levels")
            if len(c2["chunk_shape"]) != nd:
                raise LayoutError(INVALID_ARGUMENT, "chunk_shape rank")
            V.update(mid=list(c2["chunk_shape"]), index=[cfg, c2], leaf_codecs=c2["codecs"])
    V["leaf_orders"], V["leaf_a2b"], V["leaf_b2b"] = split(V["leaf_codecs"])
    if any(len(o) != nd for o in V["leaf_orders"]):
        raise LayoutError(INVALID_ARGUMENT, "transpose rank")
    if V["mid"] is not None and any(s % l for s, l in zip(V["sub"], V["mid"])):
        raise LayoutError(INVALID_ARGUMENT, "nested subchunk shape does not divide")
    if V["sub"] is not None:
        V["leaf_shape"] = V["mid"] if V["mid"] is not None else V["sub"]
    else:
        V["leaf_shape"] = list(case["descs"][0]["chunk_shape"]) if case["descs"] else [1] * nd
    return V


def index_spec(cfg, n_inner, validate):
    codecs = cfg.get("index_codecs", [{"name": "bytes", "configuration": {"endian": "little"}}, {"name": "crc32c"}])
    if codecs[0]["name"] != "bytes" or any(c["name"] != "crc32c" for c in codecs[1:]):
        raise LayoutError(UNSUPPORTED, "index_codecs must be bytes (+crc32c)")
    crcs = codecs[1:]
    if len(crcs) > 4:
        raise LayoutError(UNSUPPORTED, "too many index crc32c codecs")
    at = [int(c.get("configuration", {}).get("location") == "start") for c in crcs]
    return {"n_inner": n_inner, "index_bytes": n_inner * 16 + 4 * len(crcs),
            "at_start": int(cfg.get("index_location") == "start"),
            "big_endian": int(codecs[0]["configuration"]["endian"] == "big"), "n_crc": len(crcs),
            "crc_at_start": at + [0] * (4 - len(at)), "verify": int(validate)}


def stages(V, nelem, es):
    """Decode order: the bytes->bytes codecs last to first; a shuffle of the element size directly above the
    bytes codec is fused into the scatter. [kind, at_start, elementsize, pool], slot_bytes, n_pools, fused."""
    b2b, out, pool, slot, fused = V["leaf_b2b"], [], 0, 0, False
    for i in range(len(b2b) - 1, -1, -1):
        c, cfg = b2b[i], b2b[i].get("configuration", {})
        if c["name"] in CHECKSUMS:
            start = cfg.get("location", "start" if c["name"] == "numcodecs.adler32" else "end") == "start"
            out.append([ST[c["name"]], int(start and c["name"] != "numcodecs.fletcher32"), 0, 0])
            continue
        if c["name"] == "numcodecs.shuffle" and i == 0 and cfg.get("elementsize", 4) == es:
            fused = True
            continue
        # what this stage materialises is the chunk as the codecs before it left it: fixed-size ones only
        size = nelem * es
        for before in b2b[:i]:
            if before["name"] in CHECKSUMS:
                size += 4
            elif before["name"] != "numcodecs.shuffle":
                raise LayoutError(UNSUPPORTED, "a compressor under another variable-size codec")
        out.append([ST[c["name"]], 0, cfg.get("elementsize", 4) if c["name"] == "numcodecs.shuffle" else 0, pool])
        pool ^= 1
        slot = max(slot, size)
    n_mat = sum(1 for s in out if s[0] not in (0, 5, 6))
    return out, -(-slot // 256) * 256, min(2, n_mat), fused


def elements(case, V, i):
    """Every selected element of sharded descriptor i: (middle-shard lin, leaf lin) -> list of (position in
    the leaf, output position per encoded axis). Also returns the shard's subchunk counts."""
    nd, D = case["nd"], case["descs"][i]
    shape = D["chunk_shape"]
    dec = np.indices(shape)                                        # decoded coordinates of every element
    sel = np.ones(shape, bool)
    for d in range(nd):
        sel &= (dec[d] >= D["sel_start"][d]) & (dec[d] < D["sel_start"][d] + D["sel_shape"][d])
    out = dec - np.array(D["sel_start"]).reshape([nd] + [1] * nd) + np.array(D["out_start"]).reshape([nd] + [1] * nd)
    mo = axes_of(V["outer"], nd)
    sel_e, out_e = through(sel, V["outer"]), through(out, V["outer"], 1)
    eshape, sub, leaf = sel_e.shape, V["sub"], V["leaf_shape"]
    cps = [e // s for e, s in zip(eshape, sub)]
    cps2 = [s // l for s, l in zip(sub, leaf)]
    groups = {}
    for p in zip(*np.nonzero(sel_e)):
        if V["mid"] is not None:
            mid = np.ravel_multi_index([x // s for x, s in zip(p, sub)], cps)
            q = [x % s for x, s in zip(p, sub)]
            lin = np.ravel_multi_index([x // l for x, l in zip(q, leaf)], cps2)
        else:
            mid, q = -1, p
            lin = np.ravel_multi_index([x // l for x, l in zip(p, leaf)], cps)
        o = out_e[(slice(None),) + tuple(p)]                       # output position, decoded axis order
        groups.setdefault((int(mid), int(lin)), []).append(([x % l for x, l in zip(q, leaf)], [int(o[mo[a]]) for a in range(nd)]))
    return groups, cps


def box(group):
    """The bounding box of a leaf's elements: (sel_start, sel_shape, out_start); dense, and every element's
    offset from the box's origin the same in the leaf and in the output."""
    pos, outs = np.array([g[0] for g in group]), np.array([g[1] for g in group])
    lo, ext, o0 = pos.min(0), pos.max(0) - pos.min(0) + 1, outs.min(0)
    assert len(group) == int(np.prod(ext)), "a leaf's selection is not a dense box"
    assert ((pos - lo) == (outs - o0)).all()
    return [int(x) for x in lo], [int(x) for x in ext], [int(x) for x in o0]


def desc_status(case, V, i):
    """0, or the status a descriptor gets by itself; "skip": no elements and nothing to check."""
    nd, D, first = case["nd"], case["descs"][i], case["descs"][0]
    ok = all(D["sel_start"][d] + D["sel_shape"][d] <= D["chunk_shape"][d] and
             D["out_start"][d] + D["sel_shape"][d] <= case["out_shape"][d] for d in range(nd))
    if V["sub"] is None and list(D["chunk_shape"]) != list(first["chunk_shape"]):
        ok = False
    if not ok:
        return INVALID_ARGUMENT
    full = all(D["sel_start"][d] == 0 and D["sel_shape"][d] == D["chunk_shape"][d] for d in range(nd))
    if int(np.prod(D["sel_shape"])) == 0 and (not full or V["sub"] is not None):
        return "skip"
    return 0


def model(case):
    """The expected layout, as the fields the harness prints; raises LayoutError for a chain error."""
    nd, descs, es = case["nd"], case["descs"], ES[case["data_type"]]
    V = levels(case)
    leaf_shape = V["leaf_shape"]
    nelem = int(np.prod(leaf_shape))
    L = {"items": [], "geom": [], "item_desc_status": [0] * len(descs), "shards": [], "mids": [], "alg_bytes_static": 0}
    boxes = []  # per item: desc, sel_start, sel_shape (leaf frame), out_start, extent (output axes): check_cover
    n_inner, mo = 0, axes_of(V["outer"], nd)
    for i, D in enumerate(descs):
        st = desc_status(case, V, i)
        if st:
            L["item_desc_status"][i] = 0 if st == "skip" else st
            continue
        full = all(D["sel_start"][d] == 0 and D["sel_shape"][d] == D["chunk_shape"][d] for d in range(nd))
        L["alg_bytes_static"] += int(np.prod(D["sel_shape"])) * es  # (counted before the shard's shape is checked)
        src, ln = (0x10000 * (i + 1), 1000 + i) if D["present"] else (0, 0)
        if V["sub"] is None:
            L["items"].append([src, ln, i, (0 if D["present"] else FILL) | (0 if full else PARTIAL), 0, 0])
            L["geom"] += list(D["sel_start"]) + list(D["sel_shape"]) + list(D["out_start"])
            L["alg_bytes_static"] += ln
            boxes.append((i, D["sel_start"], D["sel_shape"], D["out_start"], D["sel_shape"]))
            continue
        eshape = [D["chunk_shape"][mo[a]] for a in range(nd)]
        if any(e % s for e, s in zip(eshape, V["sub"])):
            L["item_desc_status"][i] = INVALID_ARGUMENT
            continue
        groups, cps = elements(case, V, i)
        if n_inner and n_inner != int(np.prod(cps)):
            L["item_desc_status"][i] = UNSUPPORTED
            continue
        n_inner = int(np.prod(cps))
        slot = len(L["shards"])
        L["shards"].append([src, ln])
        flags = (SHARDED | (0 if full else PARTIAL)) if D["present"] else FILL
        for mid, grp in itertools.groupby(sorted(groups), key=lambda k: k[0]):
            at = slot
            if V["mid"] is not None:
                at = len(L["mids"])
                L["mids"].append([0, 0, i, SHARDED if D["present"] else FILL, slot, mid])
            for key in grp:
                s0, sz, o0 = box(groups[key])
                L["items"].append([0, 0, i, flags, at, key[1]])
                L["geom"] += s0 + sz + o0
                boxes.append((i, s0, sz, [o0[mo.index(d)] for d in range(nd)], [sz[mo.index(d)] for d in range(nd)]))
    L["sharded"], L["nested"] = int(V["sub"] is not None), int(V["mid"] is not None)
    zero = {"n_inner": 0, "index_bytes": 0, "at_start": 0, "big_endian": 0, "n_crc": 0, "crc_at_start": [0] * 4, "verify": 0}
    L["ispec"], L["ispec2"] = dict(zero), dict(zero)
    if V["sub"] is not None:
        L["ispec"] = index_spec(V["index"][0], n_inner, case["validate"])
        L["alg_bytes_static"] += L["ispec"]["index_bytes"] * sum(1 for s in L["shards"] if s[0])
        if V["mid"] is not None:
            L["ispec2"] = index_spec(V["index"][1], int(np.prod([s // l for s, l in zip(V["sub"], V["mid"])])), case["validate"])
            L["alg_bytes_static"] += L["ispec2"]["index_bytes"] * sum(1 for m in L["mids"] if not m[3] & FILL)
    L["stages"], L["slot_bytes"], L["n_pools"], fused = stages(V, nelem, es)
    L.update(scatter_model(case, V, L, fused))
    return L, boxes


def scatter_model(case, V, L, fused):
    nd, es, leaf_shape = case["nd"], ES[case["data_type"]], V["leaf_shape"]
    nelem, ni = int(np.prod(leaf_shape)), len(L["items"])
    geom = np.array(L["geom"], dtype=np.int64).reshape(ni, 3, nd)
    m = axes_of(V["leaf_orders"], nd)
    eshape = [leaf_shape[a] for a in m]
    if nelem:
        # the encoded chunk is a C-order array of the transposed shape; undo the transposes on its element
        # numbers and numpy's strides are the encoded stride of every decoded axis
        v = np.arange(nelem, dtype=np.int64).reshape(eshape)
        for o in reversed(V["leaf_orders"]):
            v = v.transpose(np.argsort(o))
        assert list(v.shape) == list(leaf_shape)
        enc_stride = [s // 8 for s in v.strides]
    else:
        v, enc_stride = None, [0] * nd
        for a in range(nd - 1, -1, -1):
            enc_stride[m[a]] = int(np.prod(eshape[a + 1:]))
    o = through(np.arange(int(np.prod(case["out_shape"])), dtype=np.int64).reshape(case["out_shape"]), V["outer"])
    out_stride = [s // 8 for s in o.strides] if o.size else None
    tile_a = m[nd - 1]
    others = [d for d in range(nd - 1) if d != tile_a]
    tile_b = min(others, key=lambda d: (enc_stride[d], -d)) if others else MAXD
    big = V["leaf_a2b"]["configuration"].get("endian") == "big"
    S = {"nd": nd, "es": es, "comp": COMP[case["data_type"]], "swap": int(big and COMP[case["data_type"]] > 1),
         "shuffle": int(fused), "tile_a": tile_a, "tile_b": tile_b, "pad0": case["knobs"]["unshuffle_wide"],
         "chunk_shape": list(leaf_shape), "enc_stride": enc_stride, "out_stride": out_stride, "nelem": nelem}
    outer_perm = axes_of(V["outer"], nd) != list(range(nd))
    if outer_perm and out_stride[nd - 1] != 1:
        mode = GENERIC
    elif tile_a == nd - 1:
        mode = ROWS
    elif not fused and es in (1, 2, 4, 8):
        mode = TILED
    else:
        mode = GENERIC
    max_sel = geom[:, 1, :].max(0) if ni else np.zeros(nd, np.int64)
    if not ni:
        units = 0
    elif mode == ROWS:
        units = -(-int(np.prod(max_sel[:-1])) // 64)
    elif mode == GENERIC:
        units = -(-int(np.prod(max_sel)) // 256)
    else:  # 64 x 64 tiles over (tile_a, last axis), slabs of 4 (2 for 8-byte elements) along tile_b
        tj = 2 if es == 8 else 4
        units = int(np.prod([-(-int(x) // 64) if d in (tile_a, nd - 1) else -(-int(x) // tj) if d == tile_b else int(x)
                             for d, x in enumerate(max_sel)]))
    whole = [bool((geom[i, 0] == 0).all() and (geom[i, 1] == leaf_shape).all()) for i in range(ni)]
    c_order = nelem > 0 and enc_stride == [int(np.prod(leaf_shape[d + 1:])) for d in range(nd)]
    rows_unchanged = (mode == ROWS and not S["swap"] and not fused and nelem > 0 and c_order and out_stride[nd - 1] == 1 and
                      all(out_stride[d] * es % 16 == 0 for d in range(nd - 1)))
    last = L["stages"][-1][0] if L["stages"] else None
    row_bytes = leaf_shape[nd - 1] * es
    # persistent tiled scatter: a tiled batch of whole chunks made of full tiles, every row and origin 16-B aligned
    origin = [int(sum(geom[i, 2, d] * out_stride[d] for d in range(nd))) for i in range(ni)] if ni else []
    tiled_p = (mode == TILED and ni > 0 and all(whole) and leaf_shape[tile_a] % 64 == 0 and leaf_shape[nd - 1] % 64 == 0 and
               out_stride[nd - 1] == 1 and all(x * es % 16 == 0 for x in origin) and
               all(leaf_shape[d] == 1 or ((d == tile_a or enc_stride[d] * es % 16 == 0) and
                                          (d == nd - 1 or out_stride[d] * es % 16 == 0)) for d in range(nd)))
    R = {"scatter": S, "scatter_mode": mode, "scatter_units": units, "tiled_p": int(tiled_p),
         "origin": origin if tiled_p else [], "first_path": TILED_PERSISTENT if tiled_p else mode, "no_scatter": 0}
    R["bl_direct"] = int(last == ST["blosc"] and rows_unchanged and row_bytes % 16 == 0 and not case["knobs"]["blosc_no_direct"] and
                         all(whole[i] and geom[i, 2, nd - 1] * es % 16 == 0 for i in range(ni) if not L["items"][i][3] & FILL))
    pow2 = lambda x: x & (x - 1) == 0
    R["gz_direct"] = int(last == ST["gzip"] and rows_unchanged and case["knobs"]["gzip_direct"] and nd <= 3 and
                         row_bytes >= 16 and pow2(row_bytes) and all(pow2(leaf_shape[d]) for d in range(1, nd - 1)))
    R["gz"] = ({"want": nelem * es, "nd": nd, "lbs": row_bytes.bit_length() - 1, "cshape": (list(leaf_shape) + [0] * 4)[:4],
                "ostr": ([x * es for x in out_stride] + [0] * 4)[:4]} if R["gz_direct"] else None)
    # blosc's partial decode: the encoded byte range from a partial item's first selected element to its last
    need = []
    if last == ST["blosc"] and not fused and not case["knobs"]["blosc_no_partial"]:
        for i in range(ni):
            if L["items"][i][3] & PARTIAL and geom[i, 1].all():
                picked = v[tuple(slice(int(a), int(a + n)) for a, n in zip(geom[i, 0], geom[i, 1]))]
                need += [int(picked.min()) * es, (int(picked.max()) + 1) * es]
            else:
                need += [0, -1]
        if not any(L["items"][i][3] & PARTIAL and geom[i, 1].all() for i in range(ni)):
            need = []
    R["bl_need"] = need
    return R


def check_cover(case, L, boxes):
    """The model's own sanity, without the library: every selected element of every accepted descriptor is
    covered exactly once (the cases keep their descriptors' output boxes apart), and no box reaches outside
    its leaf or the output."""
    V = levels(case)
    want = np.zeros(case["out_shape"], np.int64)
    got = np.zeros(case["out_shape"], np.int64)
    for i, D in enumerate(case["descs"]):
        if desc_status(case, V, i) == 0 and L["item_desc_status"][i] == 0:
            want[tuple(slice(o, o + n) for o, n in zip(D["out_start"], D["sel_shape"]))] += 1
    assert want.max(initial=0) <= 1, "the case's descriptors overlap in the output"
    for i, s0, sz, out_dec, ext_dec in boxes:
        assert all(a + n <= l for a, n, l in zip(s0, sz, V["leaf_shape"]))
        assert all(o + n <= l for o, n, l in zip(out_dec, ext_dec, case["out_shape"]))
        got[tuple(slice(o, o + n) for o, n in zip(out_dec, ext_dec))] += 1
    assert (got == want).all(), "selected elements are not covered exactly once"
