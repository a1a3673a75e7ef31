"""The table of the instance-norm plans (csrc/norm.hip: norm_plan; include/miseg_hip.h: miseg_instnorm_*_plan): one row per call whose
launches somebody claims to know - the case matrix of tests/instnorm_ref.py, every clause of every alignment predicate, the slab forms, the
rank-1 pair, the refusals.  Each row gives the entry point, dtype, B, S, C, the layout of every operand that is not contiguous (the names of
tests/layouts.py), the options, and what the plan must say: the return code, the predicate, and each launch as literal numbers

    (kernel, vec, cv, tx, ty, rpb, chunks, ctiles, lds_bytes[, from_slabs, rank1])

derived by hand from the launchers' rules (V = 8 bf16 / 4 fp32 elements of a 16-byte lane):

    streaming   vec = V if the predicate holds and V | C else 1; cv = C / vec; tx = min(cv, 32); ty = 256 // tx; ctiles = ceil(cv / tx);
                rpb = clamp(ceil(S / target), 4 ty, 1024) with target 256 (statistics) or 1024; chunks = ceil(S / rpb)
                LDS: reductions max(8 ty tx vec, 16 nstat tx vec), apply 16 nstat tx vec (rank-1 pair: at least 1024 vec)
    fused       ty = the power of two >= S in [16, 256]; tx = 256 // ty; vec = V halved until it divides C, then (while > 2) until
                ceil(S / ty) * vec <= 16; rpb = chunks = ctiles = 0; LDS vec tx x 144 (forward) / 160 (backward) / 248 (pair)

Nothing here computes them: tests/test_instnorm_plan_cpu.py asks the library with stand-in addresses and compares; the GPU cases of
tests/test_hip_instnorm_forms.py ask with their real operands, right beside the launch, and compare with the same rows."""
import ctypes as C

A = 1 << 12                     # a 16-byte aligned stand-in address
ES = {"bf16": 2, "fp32": 4}
NV = {"bf16": 8, "fp32": 4}
OK, BADARG, UNSUPPORTED = 0, -1, -2
NONE, LEAKY = 0, 1

ENTRY_FN = {"stats": "miseg_instnorm_stats", "apply": "miseg_instnorm_apply", "fwd": "miseg_instnorm_fwd", "fwd_slabs": "miseg_instnorm_fwd_slabs",
            "bwd": "miseg_instnorm_bwd", "bwd_apply": "miseg_instnorm_bwd_apply", "bwd_slabs": "miseg_instnorm_bwd_slabs",
            "bwd_reduce": "miseg_instnorm_bwd_reduce", "pair": "miseg_instnorm_pair_bwd"}
# the operands of each entry's alignment predicate, by the name the layouts are given under; * = optional (options switch it on)
OPERANDS = {"stats": ("x",), "apply": ("x", "y", "res*"), "fwd": ("x", "y", "res*"), "fwd_slabs": ("x", "y", "res*"),
            "bwd": ("dy", "x", "dx", "y*", "dres*", "gadd*"), "bwd_apply": ("dy", "x", "dx", "dres*", "gadd*"), "bwd_slabs": ("x", "dx", "y*", "dres*", "gadd*"),
            "bwd_reduce": ("dy", "x"), "pair": ("dy", "y*", "xa", "xb", "dxb", "dxa")}


def standin(Cc, dtype, layout):
    """(address, ld) of an operand of the given layout (tests/layouts.py::Slot: the same offsets and row strides), nothing allocated"""
    n, es = NV[dtype], ES[dtype]
    cp = -(-Cc // n) * n
    off, ld = {"contig": (0, Cc), "slice": (n, cp + 3 * n), "off8": (n // 2, cp + 2 * n), "ldodd": (0, cp + n + 1)}[layout]
    return A + off * es, ld


# ----------------------------------------------------------------------------------------------------------------- rows
ROWS = []


def row(id, entry, dtype, S, Cc, launches=(), B=2, lay=None, rc=OK, aligned=1, launch=True, **opts):
    """launches: [(kernel, vec, cv, tx, ty, rpb, chunks, ctiles, lds[, from_slabs, rank1])].  opts: res / act / y / dres / gadd / rank1 (bool: the
    optional operands), nslabs / gap / slabs_off (slab forms: slab_stride = B S C + gap, slabs 16-byte aligned + slabs_off bytes), set
    ({field: value} written into the params after they are built: the refusals), no_params / no_slabs.  launch: scripts/instnorm_table.py
    and the GPU tests may launch the row (False: a plan-only row)"""
    assert id not in {r["id"] for r in ROWS}, id
    ROWS.append({"id": id, "entry": entry, "dtype": dtype, "B": B, "S": S, "C": Cc, "lay": lay or {}, "opts": opts, "rc": rc, "aligned": aligned if rc == OK else 0,
                 "launches": [tuple(l) + (0, 0)[len(l) - 9:] for l in launches], "launch": launch and rc == OK})


def _both(entry):
    return {"stats": ("STATS",), "apply": ("APPLY",), "fwd": ("STATS", "APPLY"), "bwd": ("BWD_REDUCE", "BWD_APPLY"), "bwd_apply": ("BWD_APPLY",),
            "bwd_reduce": ("BWD_REDUCE",), "pair": ("PAIR_BWD_REDUCE", "PAIR_BWD_APPLY")}[entry]


def streaming(tag, dtype, S, Cc, geo, red, app, papp, entries=("fwd", "bwd", "pair"), B=2, **kw):
    """rows of the streaming entries at one shape: geo = (vec, cv, tx, ty, rpb, chunks, ctiles), the LDS bytes of a reduction, of an apply and
    of the pair's apply - literal numbers, the same for every entry because the geometry is"""
    for e in entries:
        lds = {"STATS": red, "APPLY": app, "BWD_REDUCE": red, "BWD_APPLY": app, "PAIR_BWD_REDUCE": red, "PAIR_BWD_APPLY": papp}
        row(f"{e}-{dtype}-S{S}-C{Cc}-{tag}", e, dtype, S, Cc, [(k,) + geo + (lds[k],) for k in _both(e)], B=B, **kw)


def fused(tag, dtype, S, Cc, geo, lds3, entries=("fwd", "bwd", "pair"), **kw):
    """rows of the one-launch entries at one shape: geo = (vec, cv, tx, ty), lds3 = the LDS bytes of forward, backward and pair backward"""
    for e in entries:
        k, lds = {"fwd": ("FUSED_FWD", lds3[0]), "bwd": ("FUSED_BWD", lds3[1]), "pair": ("PAIR_FUSED_BWD", lds3[2])}[e]
        row(f"{e}-{dtype}-S{S}-C{Cc}-{tag}", e, dtype, S, Cc, [(k,) + geo + (0, 0, 0, lds)], **kw)


ALL_STREAMING = ("stats", "apply", "fwd", "bwd", "bwd_reduce", "bwd_apply", "pair")

# ---- a. streaming geometry at S = 2049 (instnorm_ref.stream_channels)
#                                   vec cv  tx  ty  rpb chunks ctiles   reduce  apply  pair apply
streaming("tx3", "bf16", 2049, 24, (8, 3, 3, 85, 340, 7, 1), 16320, 768, 1536, entries=ALL_STREAMING)          # ty = 85: one idle thread; 7 chunks, the last 9 rows
streaming("tx3", "fp32", 2049, 12, (4, 3, 3, 85, 340, 7, 1), 8160, 384, 768, entries=ALL_STREAMING)
streaming("onetile", "bf16", 2049, 256, (8, 32, 32, 8, 32, 65, 1), 16384, 8192, 16384, entries=ALL_STREAMING)    # 65 chunks of 32 rows: every replica several times
streaming("onetile", "fp32", 2049, 128, (4, 32, 32, 8, 32, 65, 1), 8192, 4096, 8192, entries=ALL_STREAMING)
streaming("twotiles", "bf16", 2049, 320, (8, 40, 32, 8, 32, 65, 2), 16384, 8192, 16384, entries=ALL_STREAMING)   # 8 of 32 columns live in the second tile
streaming("twotiles", "fp32", 2049, 160, (4, 40, 32, 8, 32, 65, 2), 8192, 4096, 8192, entries=ALL_STREAMING)
for _dt in ("bf16", "fp32"):
    streaming("scalar1", _dt, 2049, 1, (1, 1, 1, 256, 1024, 3, 1), 2048, 32, 64, entries=ALL_STREAMING, aligned=0)          # three chunks, the last: one row
    streaming("scalar50", _dt, 2049, 50, (1, 50, 32, 8, 32, 65, 2), 2048, 1024, 2048, entries=ALL_STREAMING, aligned=0)     # scalar, two tiles, 18 live in the second
# the 1024-row cap of rows per workgroup with more chunks than either target (instnorm_ref.LONG_S = 1024^2 + 1029): 1026 chunks, the last 5 rows
streaming("rowcap", "bf16", 1024 * 1024 + 1029, 8, (8, 1, 1, 256, 1024, 1026, 1), 16384, 256, 512, entries=("stats", "apply", "bwd"), B=1)
streaming("rowcap", "fp32", 1024 * 1024 + 1029, 4, (4, 1, 1, 256, 1024, 1026, 1), 8192, 128, 256, entries=("stats", "apply", "bwd"), B=1)
# the statistics launch aims at 256 workgroups, apply / backward at 1024: 16384 rows of one full tile are 256 chunks of 64 rows beside 512 of 32
row("fwd-bf16-S16384-C256-targets", "fwd", "bf16", 16384, 256, [("STATS", 8, 32, 32, 8, 64, 256, 1, 16384), ("APPLY", 8, 32, 32, 8, 32, 512, 1, 8192)], B=1)
row("fwd-fp32-S16384-C128-targets", "fwd", "fp32", 16384, 128, [("STATS", 4, 32, 32, 8, 64, 256, 1, 8192), ("APPLY", 4, 32, 32, 8, 32, 512, 1, 4096)], B=1)
row("bwd-bf16-S16384-C256-targets", "bwd", "bf16", 16384, 256, [("BWD_REDUCE", 8, 32, 32, 8, 32, 512, 1, 16384), ("BWD_APPLY", 8, 32, 32, 8, 32, 512, 1, 8192)], B=1)

# ---- b. fused geometry (instnorm_ref.FUSED_ROWS x (V, 3), and the dead-column shapes)
#                        vec cv tx  ty     LDS fwd / bwd / pair
for _S in (2, 8, 16):                                                         # the ty floor: 16 row lanes, 16 channel columns
    fused("tyfloor", "bf16", _S, 8, (8, 1, 16, 16), (18432, 20480, 31744))
    fused("tyfloor", "fp32", _S, 4, (4, 1, 16, 16), (9216, 10240, 15872))
    for _dt in ("bf16", "fp32"):
        fused("tyfloor", _dt, _S, 3, (1, 3, 16, 16), (2304, 2560, 3968), aligned=0)      # contiguous rows of 3: ld is no whole number of lanes
for _S in (17, 27):                                                           # ty = 32
    fused("ty32", "bf16", _S, 8, (8, 1, 8, 32), (9216, 10240, 15872))
    fused("ty32", "fp32", _S, 4, (4, 1, 8, 32), (4608, 5120, 7936))
    for _dt in ("bf16", "fp32"):
        fused("ty32", _dt, _S, 3, (1, 3, 8, 32), (1152, 1280, 1984), aligned=0)
for _S in (256, 257, 512):                                                    # ty = 256, one and two rows per lane: full lanes
    fused("ty256", "bf16", _S, 8, (8, 1, 1, 256), (1152, 1280, 1984))
for _S in (256, 257, 512, 513, 1024):                                         # fp32: three and four rows of four channels are <= 16 elements per lane
    fused("ty256", "fp32", _S, 4, (4, 1, 1, 256), (576, 640, 992))
for _S in (513, 1024):                                                        # bf16 8 -> 4 at three rows per lane
    fused("lane4", "bf16", _S, 8, (4, 2, 1, 256), (576, 640, 992))
for _S in (1025, 2047, 2048):                                                 # five .. eight rows per lane: bf16 -> 2, fp32 4 -> 2 (never below 2)
    fused("lane2", "bf16", _S, 8, (2, 4, 1, 256), (288, 320, 496))
    fused("lane2", "fp32", _S, 4, (2, 2, 1, 256), (288, 320, 496))
for _S in (256, 257, 512, 513, 1024, 1025, 2047, 2048):
    for _dt in ("bf16", "fp32"):
        fused("ty256", _dt, _S, 3, (1, 3, 1, 256), (144, 160, 248), aligned=0)           # three workgroups per sample
fused("dead3of8", "bf16", 27, 40, (8, 5, 8, 32), (9216, 10240, 15872))        # tx = 8 with 5 live columns
fused("dead3of8", "fp32", 27, 20, (4, 5, 8, 32), (4608, 5120, 7936))
fused("dead15of16", "bf16", 16, 136, (8, 17, 16, 16), (18432, 20480, 31744))  # two workgroups, one live column in the second
fused("dead15of16", "fp32", 16, 68, (4, 17, 16, 16), (9216, 10240, 15872))
for _dt in ("bf16", "fp32"):
    fused("dead3of8", _dt, 27, 13, (1, 13, 8, 32), (1152, 1280, 1984), aligned=0)        # scalar 8 + 5
# lanes narrowed by divisibility: only views get here (contiguous rows of these widths have ld % V != 0): every operand an aligned slice
_SL = {"res": True, "act": True, "y": True, "dres": True, "gadd": True}
for _dt, _C, _g27, _l27, _g1000, _l1000 in (("bf16", 12, (4, 3, 8, 32), (4608, 5120, 7936), (4, 3, 1, 256), (576, 640, 992)),
                                            ("bf16", 10, (2, 5, 8, 32), (2304, 2560, 3968), (2, 5, 1, 256), (288, 320, 496)),
                                            ("fp32", 6, (2, 3, 8, 32), (2304, 2560, 3968), (2, 3, 1, 256), (288, 320, 496))):
    _lay = {k: "slice" for k in ("x", "y", "res", "dy", "dx", "dres", "gadd", "xa", "xb", "dxa", "dxb")}
    fused("slices", _dt, 27, _C, _g27, _l27, lay=_lay, **_SL)
    fused("slices", _dt, 1000, _C, _g1000, _l1000, lay=_lay, **_SL)
# the boundary between the generations, through miseg_instnorm_fwd (which decides)
fused("lastfused", "bf16", 2048, 48, (2, 24, 1, 256), (288, 320, 496))
fused("lastfused", "fp32", 2048, 48, (2, 24, 1, 256), (288, 320, 496))
fused("lastfused", "bf16", 2048, 50, (2, 25, 1, 256), (288, 320, 496), entries=("fwd",), lay={"x": "slice", "y": "slice"})      # aligned views: 50 = 2 x 25
for _dt in ("bf16", "fp32"):
    fused("lastfused-contig", _dt, 2048, 50, (1, 50, 1, 256), (144, 160, 248), aligned=0)      # contiguous: ld = 50 is no whole number of lanes

# ---- c. every clause of every alignment predicate, broken alone: 48 channels, S = 2049 (streaming) and 27 (fused where the entry has it)
#             dtype: aligned geo                 reduce apply pair    broken geo                  reduce apply pair
_CL_STREAM = {("bf16", 2049): ((8, 6, 6, 42, 168, 13, 1), 16128, 1536, 3072, (1, 48, 32, 8, 32, 65, 2), 2048, 1024, 2048),
              ("fp32", 2049): ((4, 12, 12, 21, 84, 25, 1), 8064, 1536, 3072, (1, 48, 32, 8, 32, 65, 2), 2048, 1024, 2048),
              ("bf16", 27): ((8, 6, 6, 42, 168, 1, 1), 16128, 1536, 3072, (1, 48, 32, 8, 32, 1, 2), 2048, 1024, 2048),
              ("fp32", 27): ((4, 12, 12, 21, 84, 1, 1), 8064, 1536, 3072, (1, 48, 32, 8, 32, 1, 2), 2048, 1024, 2048)}
_CL_FUSED = {"bf16": ((8, 6, 8, 32), (9216, 10240, 15872), (1, 48, 8, 32), (1152, 1280, 1984)),
             "fp32": ((4, 12, 8, 32), (4608, 5120, 7936), (1, 48, 8, 32), (1152, 1280, 1984))}
_ALLOPT = {"res": True, "act": True, "y": True, "dres": True, "gadd": True}
for _dt in ("bf16", "fp32"):
    for _S in (2049, 27):
        ga, ra, aa, pa, gb, rb, ab, pb = _CL_STREAM[(_dt, _S)]
        fa, la, fb, lb = _CL_FUSED[_dt]
        for _e in ("stats", "apply", "fwd", "bwd", "bwd_apply", "bwd_reduce", "pair"):
            _isf = _S == 27 and _e in ("fwd", "bwd", "pair")
            # the halves know no activation; the reduction reads dy and x alone
            _o = {} if _e == "bwd_reduce" else {k: v for k, v in _ALLOPT.items() if not (_e == "bwd_apply" and k in ("act", "y"))}
            for _op in OPERANDS[_e]:
                _op = _op.rstrip("*")
                for _l in ("slice", "off8", "ldodd"):
                    ok = _l == "slice"
                    if _isf:
                        fused(f"{_op}-{_l}", _dt, _S, 48, fa if ok else fb, la if ok else lb, entries=(_e,), lay={_op: _l}, aligned=int(ok), **_o)
                    elif _e == "fwd" and _op != "x" and not ok:
                        # the statistics launch of the streaming forward reads x alone: it keeps its 16-byte lanes beside a scalar apply
                        row(f"fwd-{_dt}-S{_S}-C48-{_op}-{_l}", "fwd", _dt, _S, 48, [("STATS",) + ga + (ra,), ("APPLY",) + gb + (ab,)], lay={_op: _l}, aligned=0, **_o)
                    else:
                        g, r, a, p = (ga, ra, aa, pa) if ok else (gb, rb, ab, pb)
                        streaming(f"{_op}-{_l}", _dt, _S, 48, g, r, a, p, entries=(_e,), lay={_op: _l}, aligned=int(ok), **_o)
        streaming("contig", _dt, _S, 48, ga, ra, aa, pa, entries=tuple(e for e in ALL_STREAMING if not (_S == 27 and e in ("fwd", "bwd", "pair"))))
    fused("contig", _dt, 27, 48, _CL_FUSED[_dt][0], _CL_FUSED[_dt][1])
# the streaming forward whose x is aligned and whose y is not, at three vectors: statistics in 16-byte lanes, apply in scalar ones (tx 24, ty 10)
row("fwd-bf16-S2049-C24-y-off8", "fwd", "bf16", 2049, 24, [("STATS", 8, 3, 3, 85, 340, 7, 1, 16320), ("APPLY", 1, 24, 24, 10, 40, 52, 1, 768)], lay={"y": "off8"}, aligned=0)
row("fwd-fp32-S2049-C12-y-off8", "fwd", "fp32", 2049, 12, [("STATS", 4, 3, 3, 85, 340, 7, 1, 8160), ("APPLY", 1, 12, 12, 21, 84, 25, 1, 384)], lay={"y": "off8"}, aligned=0)
# an absent optional operand constrains nothing: its ld and address are whatever the struct holds
row("apply-bf16-S2049-C24-absent-res-ignored", "apply", "bf16", 2049, 24, [("APPLY", 8, 3, 3, 85, 340, 7, 1, 768)], set={"ldres": 3})
row("bwd-bf16-S2049-C24-absent-y-dres-gadd-ignored", "bwd", "bf16", 2049, 24, [("BWD_REDUCE", 8, 3, 3, 85, 340, 7, 1, 16320), ("BWD_APPLY", 8, 3, 3, 85, 340, 7, 1, 768)],
    set={"ldy": 3, "lddres": 3, "ldgadd": 3})
# ... but the backward with an activation counts ldy even where y is NULL (the sign is recomputed): the parent's predicate, kept
row("bwd-bf16-S2049-C24-null-y-ldy-counts", "bwd", "bf16", 2049, 24, [("BWD_REDUCE", 1, 24, 24, 10, 40, 52, 1, 1920), ("BWD_APPLY", 1, 24, 24, 10, 40, 52, 1, 768)],
    act=True, set={"ldy": 3}, aligned=0)

# ---- d. the single halves below 2049 rows (no fused form), and the slab forms
row("bwd_apply-bf16-S27-C48-streaming-apply-alone", "bwd_apply", "bf16", 27, 48, [("BWD_APPLY", 8, 6, 6, 42, 168, 1, 1, 1536)])
row("bwd_reduce-bf16-S27-C48-streaming", "bwd_reduce", "bf16", 27, 48, [("BWD_REDUCE", 8, 6, 6, 42, 168, 1, 1, 16128)])
row("stats-fp32-S27-C48-streaming", "stats", "fp32", 27, 48, [("STATS", 4, 12, 12, 21, 84, 1, 1, 8064)])
row("apply-fp32-S27-C48-streaming", "apply", "fp32", 27, 48, [("APPLY", 4, 12, 12, 21, 84, 1, 1, 1536)])
#          dtype C   S     gap: geo, (fwd, bwd) LDS
_SLABS = {("bf16", 40, 27): {8: ((8, 5, 8, 32), 9216, 10240), 6: ((1, 40, 8, 32), 1152, 1280)},
          ("bf16", 40, 2048): {8: ((2, 20, 1, 256), 288, 320), 6: ((1, 40, 1, 256), 144, 160)},
          ("bf16", 13, 27): {8: ((1, 13, 8, 32), 1152, 1280), 6: ((1, 13, 8, 32), 1152, 1280)},
          ("bf16", 13, 2048): {8: ((1, 13, 1, 256), 144, 160), 6: ((1, 13, 1, 256), 144, 160)},
          ("fp32", 20, 27): {8: ((4, 5, 8, 32), 4608, 5120), 6: ((1, 20, 8, 32), 1152, 1280)},
          ("fp32", 20, 2048): {8: ((2, 10, 1, 256), 288, 320), 6: ((1, 20, 1, 256), 144, 160)},
          ("fp32", 13, 27): {8: ((1, 13, 8, 32), 1152, 1280), 6: ((1, 13, 8, 32), 1152, 1280)},
          ("fp32", 13, 2048): {8: ((1, 13, 1, 256), 144, 160), 6: ((1, 13, 1, 256), 144, 160)}}
for (_dt, _C, _S), _by_gap in _SLABS.items():
    for _gap, (_g, _lf, _lb) in _by_gap.items():
        for _n in (1, 3):
            _al = int(_gap == 8 and _C != 13)      # gap 6: slab_stride % 4 != 0; 13 channels: the slabs' row stride is no whole number of lanes
            row(f"fwd_slabs-{_dt}-S{_S}-C{_C}-{_n}slabs-gap{_gap}", "fwd_slabs", _dt, _S, _C, [("FUSED_FWD",) + _g + (0, 0, 0, _lf, 1)], nslabs=_n, gap=_gap, res=True,
                act=True, aligned=_al)
            row(f"bwd_slabs-{_dt}-S{_S}-C{_C}-{_n}slabs-gap{_gap}", "bwd_slabs", _dt, _S, _C, [("FUSED_BWD",) + _g + (0, 0, 0, _lb, 1)], nslabs=_n, gap=_gap, act=True,
                aligned=_al)
# three and four rows per lane from slabs: the 8-byte bf16 lane (the only size range that reaches it)
row("fwd_slabs-bf16-S1024-C40-2slabs-gap8", "fwd_slabs", "bf16", 1024, 40, [("FUSED_FWD", 4, 10, 1, 256, 0, 0, 0, 576, 1)], nslabs=2, gap=8)
row("bwd_slabs-bf16-S1024-C40-2slabs-gap8", "bwd_slabs", "bf16", 1024, 40, [("FUSED_BWD", 4, 10, 1, 256, 0, 0, 0, 640, 1)], nslabs=2, gap=8)
row("fwd_slabs-bf16-S27-C40-slabs-off8", "fwd_slabs", "bf16", 27, 40, [("FUSED_FWD", 1, 40, 8, 32, 0, 0, 0, 1152, 1)], nslabs=2, gap=8, slabs_off=8, aligned=0)
row("bwd_slabs-bf16-S27-C40-slabs-off8", "bwd_slabs", "bf16", 27, 40, [("FUSED_BWD", 1, 40, 8, 32, 0, 0, 0, 1280, 1)], nslabs=2, gap=8, slabs_off=8, aligned=0)
row("bwd_slabs-bf16-S27-C40-dy-ignored", "bwd_slabs", "bf16", 27, 40, [("FUSED_BWD", 8, 5, 8, 32, 0, 0, 0, 10240, 1)], nslabs=2, gap=8, set={"dy": A + 2, "lddy": 3})

# ---- e. the rank-1 pair: streaming at every size, the weight gradient's reduction sets a floor of 1024 vec bytes under the apply launch's LDS
row("pair-bf16-S27-C48-rank1", "pair", "bf16", 27, 48, [("PAIR_BWD_REDUCE", 8, 6, 6, 42, 168, 1, 1, 16128, 0, 1), ("PAIR_BWD_APPLY", 8, 6, 6, 42, 168, 1, 1, 8192, 0, 1)], rank1=True)
row("pair-fp32-S27-C48-rank1", "pair", "fp32", 27, 48, [("PAIR_BWD_REDUCE", 4, 12, 12, 21, 84, 1, 1, 8064, 0, 1), ("PAIR_BWD_APPLY", 4, 12, 12, 21, 84, 1, 1, 4096, 0, 1)], rank1=True)
# two channel tiles with one live column in the second; scalar lanes with 18 live in the second tile
row("pair-bf16-S2049-C264-rank1", "pair", "bf16", 2049, 264, [("PAIR_BWD_REDUCE", 8, 33, 32, 8, 32, 65, 2, 16384, 0, 1), ("PAIR_BWD_APPLY", 8, 33, 32, 8, 32, 65, 2, 16384, 0, 1)],
    rank1=True)
row("pair-fp32-S2049-C132-rank1", "pair", "fp32", 2049, 132, [("PAIR_BWD_REDUCE", 4, 33, 32, 8, 32, 65, 2, 8192, 0, 1), ("PAIR_BWD_APPLY", 4, 33, 32, 8, 32, 65, 2, 8192, 0, 1)],
    rank1=True)
for _dt in ("bf16", "fp32"):
    row(f"pair-{_dt}-S2049-C50-rank1", "pair", _dt, 2049, 50, [("PAIR_BWD_REDUCE", 1, 50, 32, 8, 32, 65, 2, 2048, 0, 1), ("PAIR_BWD_APPLY", 1, 50, 32, 8, 32, 65, 2, 2048, 0, 1)],
        rank1=True, aligned=0)
# C % V == 0 is a clause of the rank-1 pair's predicate of its own: aligned slices of 12 bf16 channels keep the predicate without the shortcut
_PS = {k: "slice" for k in ("dy", "xa", "xb", "dxa", "dxb")}
row("pair-bf16-S2049-C12-slices-rank1", "pair", "bf16", 2049, 12, [("PAIR_BWD_REDUCE", 1, 12, 12, 21, 84, 25, 1, 2016, 0, 1), ("PAIR_BWD_APPLY", 1, 12, 12, 21, 84, 25, 1, 1024, 0, 1)],
    rank1=True, lay=_PS, aligned=0)
row("pair-bf16-S2049-C12-slices", "pair", "bf16", 2049, 12, [("PAIR_BWD_REDUCE", 1, 12, 12, 21, 84, 25, 1, 2016), ("PAIR_BWD_APPLY", 1, 12, 12, 21, 84, 25, 1, 768)], lay=_PS)
row("apply-bf16-S2049-C24-rank1", "apply", "bf16", 2049, 24, [("APPLY", 8, 3, 3, 85, 340, 7, 1, 768, 0, 1)], rank1=True)
# the fused forward never looks at r1x (the streaming one refuses it without res_stat: below)
row("fwd-bf16-S27-C48-r1x-ignored", "fwd", "bf16", 27, 48, [("FUSED_FWD", 8, 6, 8, 32, 0, 0, 0, 9216)], set={"r1x": A}, launch=False)

# ---- f. every refusal, with its code
def refusal(id, entry, rc, S=27, dtype="bf16", Cc=16, **opts):
    row(id, entry, dtype, S, Cc, rc=rc, B=1, **opts)


refusal("stats-null-params", "stats", BADARG, no_params=True)
refusal("stats-null-x", "stats", BADARG, set={"x": 0})
refusal("stats-null-stat", "stats", BADARG, set={"stat": 0})
refusal("stats-B0", "stats", BADARG, set={"B": 0})
refusal("stats-S0", "stats", BADARG, set={"S": 0})
refusal("stats-C0", "stats", BADARG, set={"C": 0})
refusal("stats-ld-below-C", "stats", BADARG, set={"ldx": 15})
refusal("stats-dtype", "stats", BADARG, set={"dtype": 7})
refusal("apply-null-params", "apply", BADARG, no_params=True)
refusal("apply-null-y", "apply", BADARG, set={"y": 0})
refusal("apply-styles0", "apply", BADARG, set={"num_styles": 0})
refusal("apply-styles5", "apply", BADARG, set={"num_styles": 5})
refusal("apply-act-gelu", "apply", UNSUPPORTED, set={"act": 2})
refusal("apply-res_stat-without-res", "apply", BADARG, set={"res_stat": A})
refusal("apply-r1x-without-res_stat", "apply", BADARG, set={"r1x": A, "r1w": A})
refusal("apply-r1x-with-res", "apply", BADARG, rank1=True, set={"res": A})
refusal("apply-r1x-without-r1w", "apply", BADARG, rank1=True, set={"r1w": 0})
refusal("apply-dtype", "apply", BADARG, set={"dtype": 7})
refusal("apply-C0", "apply", BADARG, set={"C": 0})               # the parent divided by zero here
refusal("fwd-null-params", "fwd", BADARG, no_params=True)
refusal("fwd-null-stat", "fwd", BADARG, set={"stat": 0})
refusal("fwd-res_stat", "fwd", UNSUPPORTED, res=True, set={"res_stat": A})
refusal("fwd-fused-styles0", "fwd", BADARG, set={"num_styles": 0})
refusal("fwd-fused-act-gelu", "fwd", UNSUPPORTED, set={"act": 2})
refusal("fwd-fused-dtype", "fwd", BADARG, set={"dtype": 7})
refusal("fwd-fused-B0", "fwd", BADARG, set={"B": 0})             # the parent launched an empty grid here (MISEG_E_LAUNCH)
refusal("fwd-streaming-ld-below-C", "fwd", BADARG, S=2049, set={"ldx": 15})      # the refusals of its halves: miseg_instnorm_stats' ...
refusal("fwd-streaming-dtype", "fwd", BADARG, S=2049, set={"dtype": 7})
refusal("fwd-streaming-styles0", "fwd", BADARG, S=2049, set={"num_styles": 0})   # ... and miseg_instnorm_apply's
refusal("fwd-streaming-act-gelu", "fwd", UNSUPPORTED, S=2049, set={"act": 2})
refusal("fwd-streaming-r1x", "fwd", BADARG, S=2049, set={"r1x": A})
refusal("fwd_slabs-null-slabs", "fwd_slabs", BADARG, nslabs=1, gap=0, no_slabs=True)
refusal("fwd_slabs-S2049", "fwd_slabs", UNSUPPORTED, S=2049, nslabs=1, gap=0)
refusal("fwd_slabs-nslabs0", "fwd_slabs", BADARG, nslabs=0, gap=0)
refusal("fwd_slabs-stride-short", "fwd_slabs", BADARG, nslabs=2, gap=-1)
refusal("fwd_slabs-res_stat", "fwd_slabs", UNSUPPORTED, nslabs=1, gap=0, res=True, set={"res_stat": A})
refusal("bwd-null-params", "bwd", BADARG, no_params=True)
refusal("bwd-null-dy", "bwd", BADARG, set={"dy": 0})
refusal("bwd-null-dx", "bwd", BADARG, set={"dx": 0})
refusal("bwd-null-dstat", "bwd", BADARG, set={"dstat": 0})
refusal("bwd-act-gelu", "bwd", BADARG, set={"act": 2})           # BADARG where the forward says UNSUPPORTED: kept
refusal("bwd-styles0", "bwd", BADARG, set={"num_styles": 0})
refusal("bwd-dtype", "bwd", BADARG, set={"dtype": 7})
refusal("bwd-streaming-act-gelu", "bwd", BADARG, S=2049, set={"act": 2})
refusal("bwd_apply-null-params", "bwd_apply", UNSUPPORTED, no_params=True)      # its first check names the activation: kept
refusal("bwd_apply-act", "bwd_apply", UNSUPPORTED, set={"act": 1})
refusal("bwd_apply-null-dx", "bwd_apply", BADARG, set={"dx": 0})
refusal("bwd_slabs-null-slabs", "bwd_slabs", BADARG, nslabs=1, gap=0, no_slabs=True)
refusal("bwd_slabs-S2049", "bwd_slabs", UNSUPPORTED, S=2049, nslabs=1, gap=0)
refusal("bwd_slabs-nslabs0", "bwd_slabs", BADARG, nslabs=0, gap=0)
refusal("bwd_slabs-stride-short", "bwd_slabs", BADARG, nslabs=2, gap=-1)
refusal("bwd_reduce-null-params", "bwd_reduce", BADARG, no_params=True)
refusal("bwd_reduce-null-dy", "bwd_reduce", BADARG, set={"dy": 0})
refusal("bwd_reduce-act", "bwd_reduce", UNSUPPORTED, set={"act": 1})
refusal("bwd_reduce-dtype", "bwd_reduce", BADARG, set={"dtype": 7})
refusal("pair-null-params", "pair", BADARG, no_params=True)
refusal("pair-null-dxa", "pair", BADARG, set={"dxa": 0})
refusal("pair-null-dstat_b", "pair", BADARG, set={"dstat_b": 0})
refusal("pair-no-xb-no-r1x", "pair", BADARG, set={"xb": 0})
refusal("pair-r1x-with-xb", "pair", BADARG, set={"r1x": A, "r1w": A, "r1dw": A})
refusal("pair-r1x-with-y", "pair", BADARG, rank1=True, set={"y": A})
refusal("pair-r1x-without-r1dw", "pair", BADARG, rank1=True, set={"r1dw": 0})
refusal("pair-styles0", "pair", BADARG, set={"num_styles": 0})
refusal("pair-dtype", "pair", BADARG, set={"dtype": 7})

BY_ID = {r["id"]: r for r in ROWS}

# every (kernel, vec, from_slabs) the launchers can instantiate: the streaming kernels at V and 1, the fused ones at every halving, the
# forward and the single backward also from slabs
UNREACHABLE = {}      # (kernel, dtype, vec, from_slabs) -> why no call gets there; empty: the planner reaches every instantiation


def instantiations():
    out = set()
    for dt, V in NV.items():
        for k in ("STATS", "APPLY", "BWD_REDUCE", "BWD_APPLY", "PAIR_BWD_REDUCE", "PAIR_BWD_APPLY"):
            out |= {(k, dt, V, 0), (k, dt, 1, 0)}
        v = V
        while v >= 1:
            out |= {("FUSED_FWD", dt, v, 0), ("FUSED_FWD", dt, v, 1), ("FUSED_BWD", dt, v, 0), ("FUSED_BWD", dt, v, 1), ("PAIR_FUSED_BWD", dt, v, 0)}
            v //= 2
    return out


# ----------------------------------------------------------------------------------------------------------------- asking the library
def kernel_id(L, name):
    return getattr(L, "IN_" + name)


def _styles(L):
    return (C.c_void_p * L.MAX_STYLES)()


def params(r, L, operands=None):
    """(params struct or None, extra args) of the row's call.  operands: {name: (address, ld)} of real tensors (scripts/instnorm_table.py); default:
    stand-ins in the row's layouts.  Statistics, affine rows and the rank-1 vectors are the stand-in A unless `operands` names them."""
    o, dt, B, S, Cc = r["opts"], r["dtype"], r["B"], r["S"], r["C"]
    e = r["entry"]
    given = operands or {}

    def op(name, present=True):
        if not present:
            return 0, 0
        if operands is not None:
            return given[name]      # real operands: a missing one is an error, never a stand-in address
        return standin(Cc, dt, r["lay"].get(name, "contig"))

    def aux(name, present=True):
        if not present:
            return 0
        return given[name][0] if operands is not None else A

    dtype = {"fp32": L.F32, "bf16": L.BF16}[dt]
    act = LEAKY if o.get("act") else NONE
    r1 = bool(o.get("rank1"))
    if e == "stats":
        p = L.InstnormStats(*op("x"), B, S, Cc, dtype, aux("stat"))
    elif e in ("apply", "fwd", "fwd_slabs"):
        p = L.InstnormApply(*op("x"), *op("res", o.get("res")), *op("y"), B, S, Cc, dtype, aux("stat"), 1e-5, 0, 1, _styles(L), _styles(L), act, 0.01,
                            aux("res_stat", r1), _styles(L), _styles(L), aux("r1x", r1), 1, aux("r1w", r1))
    elif e in ("bwd", "bwd_apply", "bwd_slabs", "bwd_reduce"):
        p = L.InstnormBwd(*op("dy", e != "bwd_slabs"), *op("y", o.get("y")), *op("x"), *op("dx", e != "bwd_reduce"), *op("dres", o.get("dres")), B, S, Cc, dtype, aux("stat"), 1e-5,
                          aux("dstat"), 0, 1, _styles(L), _styles(L), _styles(L), act, 0.01, *op("gadd", o.get("gadd")), _styles(L))
    else:
        p = L.InstnormPairBwd(*op("dy"), *op("y", o.get("y") and not r1), *op("xa"), *op("xb", not r1), *op("dxa"), *op("dxb", not r1), B, S, Cc, dtype, aux("stat_a"),
                              aux("stat_b"), 1e-5, aux("dstat_a"), aux("dstat_b"), 0, 1, _styles(L), _styles(L), _styles(L), _styles(L), _styles(L), _styles(L), 0.01,
                              _styles(L), _styles(L), aux("r1x", r1), 1, aux("r1w", r1), aux("r1dw", r1))
    for k, v in o.get("set", {}).items():
        setattr(p, k, v)
    extra = ()
    if e in ("fwd_slabs", "bwd_slabs"):
        slabs = None if o.get("no_slabs") else A + o.get("slabs_off", 0)      # real slabs: the caller replaces extra[0]
        extra = (C.c_void_p(slabs), o["nslabs"], B * S * Cc + o["gap"])
    return (None if o.get("no_params") else p), extra


def ask(L, entry, p, extra=()):
    """(return code, plan) of miseg_instnorm_<entry>_plan"""
    pl = L.InstnormPlan()
    rc = getattr(L.load(), ENTRY_FN[entry] + "_plan")(C.byref(p) if p is not None else None, *extra, C.byref(pl))
    return rc, pl


def launches(L, pl):
    """the plan's launches in the table's notation"""
    names = {getattr(L, k): k[3:] for k in dir(L) if k.startswith("IN_") and isinstance(getattr(L, k), int)}
    return [(names[l.kernel], l.vec, l.cv, l.tx, l.ty, l.rpb, l.chunks, l.ctiles, l.lds_bytes, l.from_slabs, l.rank1) for l in list(pl.launch)[:pl.n_launches]]


def check_plan(r, L, rc, pl):
    assert rc == r["rc"], f"{r['id']}: the plan returns {rc}, the table says {r['rc']} ({L.load().miseg_last_error()})"
    assert launches(L, pl) == r["launches"], f"{r['id']}: the plan names {launches(L, pl)}, the table says {r['launches']}"
    assert pl.aligned == r["aligned"], f"{r['id']}: aligned {pl.aligned}, the table says {r['aligned']}"
    for l in list(pl.launch)[:pl.n_launches]:
        grid = (l.grid_x, l.grid_y, l.grid_z)
        assert grid == ((l.chunks, r["B"], l.ctiles) if l.rpb else (-(-l.cv // l.tx), r["B"], 1)), f"{r['id']}: grid {grid}"
        assert l.threads == 256 and l.tx * l.ty <= 256 and r["C"] % l.vec == 0 and l.cv * l.vec == r["C"], r["id"]


def find(entry, dtype, S, Cc, tag=None):
    """the id of the row of this call: with its tag, or - tag None - the one row of that entry, dtype and shape"""
    head = f"{entry}-{dtype}-S{S}-C{Cc}-"
    ids = [head + tag] if tag is not None else [i for i in BY_ID if i.startswith(head)]
    assert len(ids) == 1 and ids[0] in BY_ID, f"no single row for {head}{tag or '*'}: {ids}"
    return ids[0]


def assert_plan(L, id, p, extra=()):
    """beside a launch: the plan of this very call - real operands - is what the table's row says"""
    r = BY_ID[id]
    rc, pl = ask(L, r["entry"], p, extra)
    check_plan(r, L, rc, pl)
