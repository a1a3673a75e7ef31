"""Cases of the attention launch plan (miseg_winattn_fwd_plan / miseg_winattn_bwd_plan) for tests/test_winattn_plan_cpu.py and
scripts/winattn_answer_digest.py: parameter structs with stand-in pointers, the table of rows with the plan fields worked out by hand from
the dispatcher as it was before the plan existed (csrc/attention.hip: make_geom, fwd_takes_mfma, bwd_takes_mfma, the launchers' vec / wide
expressions; csrc/attention_global.hip: ga_geom, ga_bwd_geom and the two launchers), the sets of kernel instantiations, and a seeded sweep
over the two question entry points.  The specs are those tests/test_hip_winattn_forms.py launches (tests/winattn_ref.py).  CPU only."""
import hashlib
import os
import re
import struct

import torch

import winattn_ref as W

S = W.Spec
A = 1 << 12      # an aligned stand-in address: the plan reads pointers for NULL and alignment only
BADARG, UNSUPPORTED = -1, -2
NONE, QUERY_LANE, WINDOW, GLOBAL = range(4)      # miseg_winattn_plan_info.kernel
F32, BF16 = 0, 1      # MISEG_F32 / MISEG_BF16
OPERANDS = ("qkv", "out", "dout", "dqkv")
# tests/layouts.py, rows of c channels (c a multiple of N = 16 bytes of elements): layout -> (offset of the view, row stride beyond c) in units of N
# (ldodd: one element more)
LAYOUTS = {"contig": (0, 0, 0), "slice": (1, 3, 0), "off8": (0.5, 2, 0), "ldodd": (0, 1, 1)}
QUESTIONS = ("miseg_winattn_on_matrix_cores", "miseg_winattn_bwd_on_matrix_cores")


def params(L, spec, dt=BF16, drop_p=0.0, lay=None, dtable=True, dqb=True, tw=None, null=(), off=None, slack=None):
    """(miseg_winattn_params, miseg_winattn_bwd_params) of a Spec.  lay: {operand: layout}; off / slack: {operand: byte offset / extra row
    stride in elements} directly; dtable / dqb: the parameter gradients are asked for (dtable "force": also without a table); null: operands
    handed in as NULL"""
    es = 2 if dt == BF16 else 4
    lay, off, slack = lay or {}, dict(off or {}), dict(slack or {})
    for o, name in lay.items():
        e, s, odd = LAYOUTS[name]
        off[o], slack[o] = int(e * 16), s * (16 // es) + odd
    ptr = {o: (None if o in null else A + off.get(o, 0)) for o in OPERANDS + ("lse",)}
    ld = {o: (3 if o in ("qkv", "dqkv") else 1) * spec.C + slack.get(o, 0) for o in OPERANDS}
    f = L.Winattn(ptr["qkv"], ld["qkv"], ptr["out"], ld["out"], A if spec.bias else None, A if spec.table else None, ptr["lse"], spec.B, *spec.dims, spec.C,
                  spec.heads, dt, *spec.ws, *spec.ss, spec.tw if tw is None else tw, spec.scale, drop_p, 0x5EED, 11, A)
    want_dtable = dtable == "force" or (dtable and spec.table)
    b = L.WinattnBwd(f, ptr["dout"], ld["dout"], ptr["dqkv"], ld["dqkv"], A if (dqb and spec.bias) else None, A if want_dtable else None)
    return f, b


def answers(so, f, b):
    import ctypes as C
    return so.miseg_winattn_on_matrix_cores(C.byref(f)), so.miseg_winattn_bwd_on_matrix_cores(C.byref(b))


# ---- LDS of the three kernel families, from their layouts
def ql_lds(n, hd, tsize, bwd):
    """query-lane kernels (carve): K and V rows in fp32, the table (and its gradient bins in the backward), five words per token, the
    gradient row of the padded tokens"""
    return 4 * (2 * n * hd + tsize * (2 if bwd else 1) + 5 * n + 3 * hd)


WIN_FWD_LDS = {7: 38272 + 4 * 2197, 8: 38272 + 4 * 3375, 16: 38272 + 4 * 29791}      # Q, K [352][16] and V^T [16][360] in bf16, three words per token, the table of tw
WIN_BWD_LDS = 81216      # 8 waves: three [352][16] images, five words per token, 2 x 8 dQ tiles of 1 KB, 8 dS tiles of 768 B, 64 words, 2 x 2200 table words
GLOBAL_LDS = {2: (9728, 19712), 4: (18432, 37376), 6: (27136, 55040), 8: (35840, 72704), 10: (44544, 90368), 12: (53248, 108032), 14: (61952, 125696),
              16: (70656, 143360)}      # tiles -> (forward, backward): NP rows of 72 and 64 rows of NP + 8 bf16; backward the "dK,dV" role's two of each + 2 NP words


def ql(hd4, waves):
    return ("ql", hd4, waves)


def win(waves, vec=1):
    return ("win", waves, vec)


def glob(tiles, grid_x):
    return ("glob", tiles, grid_x)


def no(rc, fragment):
    return ("rc", rc, fragment)


def expected(spec, dt, exp, bwd, drop_p, dtable, tw=None):
    """the plan fields a row's short form stands for: mask / drop / table_grad restate the request, grids and units come from the Spec"""
    tw = spec.tw if tw is None else tw
    tsize = (2 * tw - 1) ** 3 if spec.table else 0
    if exp[0] == "rc":
        return dict(rc=exp[1], kernel=NONE, units=0, grid_x=0, threads=0, lds_bytes=0)
    e = dict(mask=int(any(spec.ss)), drop=int(round(drop_p * 65536) > 0),      # p is quantised to 1 / 65536
              table_grad=int(bool(bwd and dtable and spec.table)), tokens=spec.n)
    if exp[0] == "ql":
        e.update(kernel=QUERY_LANE, hd4=exp[1], waves=exp[2], threads=64 * exp[2], tiles=0, vec=0, grid_x=spec.windows, grid_y=spec.heads, grid_z=1,
                 units=spec.windows * spec.heads, table_size=tsize, lds_bytes=ql_lds(spec.n, spec.hd, tsize, bwd))
    elif exp[0] == "win":
        e.update(kernel=WINDOW, hd4=0, waves=exp[1], threads=64 * exp[1], tiles=0, vec=exp[2], grid_x=spec.windows * spec.heads, grid_y=1, grid_z=1,
                 units=spec.windows * spec.heads, table_size=tsize, lds_bytes=WIN_BWD_LDS if bwd else WIN_FWD_LDS[tw])
    else:
        e.update(kernel=GLOBAL, hd4=0, waves=4, threads=256, tiles=exp[1], vec=0, grid_x=exp[2], grid_y=spec.heads, grid_z=spec.B, units=exp[2] * spec.heads * spec.B,
                 table_size=0, lds_bytes=GLOBAL_LDS[exp[1]][bwd])
    return e


# ================================================================================================ the rows
# (id, spec, dtype, keywords of params(), forward plan, backward plan): ql(hd4, waves) / win(waves, vec) / glob(tiles, grid_x) / no(rc, text).
# Worked out from the parent's dispatcher:
#   global: bf16, no table, head_dim 64, one unshifted window = the grid, <= 256 tokens, qkv 16-byte rows, out 8-byte pieces (backward: also dO
#     and O 16-byte rows, dqkv 8-byte pieces); tiles = ceil(n / 32) * 2, grid_x = ceil(n / 64) (backward twice that);
#   then the query-lane LDS bound of 160 KB;
#   window matrix cores: bf16, head_dim 16, a table, n <= 352; forward: out in 8-byte pieces, 11 waves below 256 units, else 8, vec = qkv in
#     16-byte rows; backward: (2 tw - 1)^3 <= 2200, qkv and dqkv in 8-byte pieces, 8 waves, vec = qkv, out, dO in 16-byte rows;
#   query lanes otherwise: hd4 = head_dim / 4 of 1, 2, 3, 4, 8, 16, waves = ceil(n / 64).
ROWS = []


def _row(id_, spec, dt, fwd, bwd, **kw):
    ROWS.append((id_, spec, dt, kw, fwd, bwd))


def _w(n):
    return -(-n // 64)


# ---- every Spec of the GPU file's GEOMETRY, in each of its dtypes: fp32 always on the query lanes (head_dim 16 throughout: hd4 = 4)
_GEOMETRY_BF16 = {      # str(spec) -> (forward, backward) in bf16
    "B2-14x14x7-w7x7x7-s3x3x0-h2c32": (win(11), win(8)), "B2-7x14x14-w7x7x7-s0x3x3-h2c32": (win(11), win(8)), "B2-14x7x4-w7x7x4-s3x0x0-h2c32": (win(11), win(8)),
    "B2-7x7x4-w7x7x4-s0x0x0-h3c48": (win(11), win(8)), "B2-4x7x7-w4x7x7-s0x0x0-h3c48": (win(11), win(8)),
    "B2-8x8x8-w4x4x4-s2x2x2-h4c64": (win(11), win(8)), "B2-8x8x8-w4x4x4-s0x0x0-h4c64": (win(11), win(8)), "B2-4x4x2-w4x4x2-s0x0x0-h1c16": (win(11), win(8)),
    "B2-8x8x5-w8x8x5-s0x0x0-h1c16": (win(11), win(8)), "B2-8x8x6-w4x4x3-s2x2x1-h2c32": (win(11), win(8)),
    "B2-3x3x3-w3x3x3-s0x0x0-h2c32": (win(11), win(8)), "B2-6x6x6-w3x3x3-s1x1x1-h2c32": (win(11), win(8)), "B2-4x4x4-w2x2x2-s1x1x1-h1c16": (win(11), win(8)),
    "B2-8x7x7-w7x7x7-s0x0x0-h3c48": (win(11), win(8)), "B2-9x5x6-w4x4x4-s2x2x2-h2c32": (win(11), win(8)),
    "B2-8x7x7-w7x7x7-s0x0x0-h3c48-nobias": (win(11), win(8)), "B2-9x5x6-w4x4x4-s2x2x2-h2c32-nobias": (win(11), win(8)),
    # n = 352 with a 15^3 table: the backward's 2200-word slots do not hold 3375 entries; 384 and 360 tokens: above 352
    "B2-11x8x4-w11x8x4-s0x0x0-h1c16-tw8": (win(11), ql(4, 6)), "B2-6x8x8-w6x8x8-s0x0x0-h1c16-tw8": (ql(4, 6), ql(4, 6)), "B2-6x6x10-w6x6x10-s0x0x0-h1c16-tw8": (ql(4, 6), ql(4, 6)),
    "B1-7x7x7-w7x7x7-s0x0x0-h1c16": (win(11), win(8)), "B1-21x21x21-w7x7x7-s3x3x3-h1c16": (win(11), win(8)), "B3-7x7x7-w7x7x7-s0x0x0-h3c48": (win(11), win(8)),
    "B1-33x20x19-w7x7x7-s3x3x3-h6c96": (win(8), win(8)),      # 270 units
    "B1-16x16x16-w4x4x4-s2x2x2-h4c64": (win(8), win(8)), "B1-16x16x12-w4x4x4-s2x2x2-h4c64": (win(11), win(8)),      # 256 and 192 units
    "B2-10x9x8-w7x7x7-s3x3x3-h2c32-amp4": (win(11), win(8)),
}
for _s, _dts in W.GEOMETRY:
    for _dt in _dts:
        if _dt == torch.float32:
            _row(f"geometry-fp32-{_s}", _s, F32, ql(4, _w(_s.n)), ql(4, _w(_s.n)))
        else:
            _row(f"geometry-bf16-{_s}", _s, BF16, *_GEOMETRY_BF16[str(_s)])

# ---- the options: dropout x table gradient x dqkv_bias on the two option specs (bf16 backward: mask x DT x DROP = the eight forms)
for _s in W.OPTION_SPECS:
    for _p in (0.0, 0.25):
        for _dtab, _dqb in ((True, True), (False, True), (True, False), (False, False)):
            _id = f"{_s}-p{_p:g}-dtable{int(_dtab)}-dqb{int(_dqb)}"
            _row("options-bf16-" + _id, _s, BF16, win(11), win(8), drop_p=_p, dtable=_dtab, dqb=_dqb)
            _row("options-fp32-" + _id, _s, F32, ql(4, _w(_s.n)), ql(4, _w(_s.n)), drop_p=_p, dtable=_dtab, dqb=_dqb)

# ---- head dims of the query-lane kernels: 8, 12, 32, 64 with a table, bf16 16 without one
for (_s, _dts), _hd4 in zip(W.HEAD_DIMS, (2, 3, 8, 16, 4)):
    for _dt in _dts:
        _row(f"head-dims-{'fp32' if _dt == torch.float32 else 'bf16'}-{_s}", _s, F32 if _dt == torch.float32 else BF16, ql(_hd4, _w(_s.n)), ql(_hd4, _w(_s.n)))

# ---- the global kernels: n = 80, 150, 180, 1, 2 -> tiles 6, 10, 12, 2, 2; grid_x = ceil(n / 64), twice that in the backward
for _s, (_t, _g) in zip(W.GLOBAL, ((6, 2), (10, 3), (12, 3), (2, 1), (2, 1))):
    for _p in (0.0, 0.1):
        _row(f"global-{_s}-p{_p:g}", _s, BF16, glob(_t, _g), glob(_t, 2 * _g), drop_p=_p)
    _row(f"global-fp32-{_s}", _s, F32, ql(16, _w(_s.n)), ql(16, _w(_s.n)))      # fp32: never the matrix cores
for _p in (0.0, 0.1):
    _row(f"global-above-p{_p:g}", W.GLOBAL_ABOVE, BF16, ql(16, 5), ql(16, 5), drop_p=_p)      # 288 tokens > 256
_G = lambda d, B=1, heads=1, **kw: S(d, d, (0, 0, 0), heads, 64 * heads, B=B, bias=False, table=False, **kw)
_row("global-n256", _G((4, 8, 8)), BF16, glob(16, 4), glob(16, 8))
_row("global-n257", _G((257, 1, 1)), BF16, ql(16, 5), ql(16, 5))
_row("global-n40-tiles4", _G((2, 4, 5), B=2, heads=3), BF16, glob(4, 1), glob(4, 2), drop_p=0.1)
_row("global-n100-tiles8", _G((4, 5, 5)), BF16, glob(8, 2), glob(8, 4))
_row("global-n200-tiles14", _G((5, 5, 8), heads=12), BF16, glob(14, 4), glob(14, 8), drop_p=0.1)
_row("global-n216-the-vit", _G((6, 6, 6), B=2, heads=12), BF16, glob(14, 4), glob(14, 8))
# (3) head_dim 64 without a table but with a shift, or a window smaller than the grid: the query lanes
_row("global-shape-shifted", S((4, 4, 5), (4, 4, 5), (1, 0, 0), 1, 64, B=1, bias=False, table=False), BF16, ql(16, 2), ql(16, 2))
_row("global-shape-window-smaller-than-grid", S((4, 4, 10), (4, 4, 5), (0, 0, 0), 1, 64, B=1, bias=False, table=False), BF16, ql(16, 2), ql(16, 2))
_row("global-shape-with-a-table", S((4, 4, 5), (4, 4, 5), (0, 0, 0), 1, 64, B=1, bias=False), BF16, ql(16, 2), ql(16, 2))
_row("global-shape-head-dim-32", S((4, 4, 5), (4, 4, 5), (0, 0, 0), 2, 64, B=1, bias=False, table=False), BF16, ql(8, 2), ql(8, 2))

# ---- layouts of the window kernels (bf16 10x9x8 in windows of 7^3, 32 units): slice changes nothing; off8 (8-byte aligned, ld % 8 == 0)
# keeps the matrix cores with scalar loads where the operand is read through the staging loads; ldodd (ld % 4 != 0) on `out` sends the
# forward to the query lanes (8-byte stores), on qkv / dqkv the backward (8-byte loads / stores)
_LAY = {("qkv", "slice"): (win(11), win(8)), ("qkv", "off8"): (win(11, 0), win(8, 0)), ("qkv", "ldodd"): (win(11, 0), ql(4, 6)),
        ("out", "slice"): (win(11), win(8)), ("out", "off8"): (win(11), win(8, 0)), ("out", "ldodd"): (ql(4, 6), win(8, 0)),
        ("dout", "slice"): (win(11), win(8)), ("dout", "off8"): (win(11), win(8, 0)), ("dout", "ldodd"): (win(11), win(8, 0)),
        ("dqkv", "slice"): (win(11), win(8)), ("dqkv", "off8"): (win(11), win(8)), ("dqkv", "ldodd"): (win(11), ql(4, 6))}
for (_o, _l), (_f, _b) in _LAY.items():
    _row(f"layout-bf16-{_o}-{_l}", W.LAYOUT_SPEC, BF16, _f, _b, lay={_o: _l})
    _row(f"layout-fp32-{_o}-{_l}", W.LAYOUT_SPEC, F32, ql(4, 6), ql(4, 6), lay={_o: _l})
for _o in ("qkv", "out", "dqkv"):
    _row(f"cross-kernel-pair-{_o}-ldodd-p0.25", W.LAYOUT_SPEC, BF16, *_LAY[(_o, "ldodd")], lay={_o: "ldodd"}, drop_p=0.25)
# ... and of the global kernels (4x4x5, one head): qkv binds both, out's 16-byte rows, dO and dqkv the backward alone
_GL = {("qkv", "ldodd"): (ql(16, 2), ql(16, 2)), ("qkv", "off8"): (ql(16, 2), ql(16, 2)), ("out", "off8"): (glob(6, 2), ql(16, 2)), ("out", "ldodd"): (ql(16, 2), ql(16, 2)),
       ("dout", "off8"): (glob(6, 2), ql(16, 2)), ("dout", "ldodd"): (glob(6, 2), ql(16, 2)), ("dqkv", "off8"): (glob(6, 2), glob(6, 4)), ("dqkv", "ldodd"): (glob(6, 2), ql(16, 2))}
for (_o, _l), (_f, _b) in _GL.items():
    for _p in (0.0, 0.1):
        _row(f"global-layout-{_o}-{_l}-p{_p:g}", W.GLOBAL_LAYOUT, BF16, _f, _b, lay={_o: _l}, drop_p=_p)

# ---- the production window shapes of the bench nets (bf16, 7^3 windows, head_dim 16): 96^3 patch stages and the deep stages below 256 units
_row("production-stage1-48x48x48", S((48, 48, 48), (7, 7, 7), (3, 3, 3), 3, 48, B=1), BF16, win(8), win(8))      # 343 windows x 3
_row("production-stage1-unshifted", S((48, 48, 48), (7, 7, 7), (0, 0, 0), 3, 48, B=1), BF16, win(8), win(8))
_row("production-stage2-24x24x24", S((24, 24, 24), (7, 7, 7), (3, 3, 3), 6, 96, B=1), BF16, win(8), win(8))      # 64 x 6 = 384
_row("production-stage3-12x12x12", S((12, 12, 12), (7, 7, 7), (3, 3, 3), 12, 192, B=1), BF16, win(11), win(8))      # 8 x 12 = 96
_row("production-stage4-6x6x6", S((6, 6, 6), (6, 6, 6), (0, 0, 0), 24, 384, B=1), BF16, win(11), win(8))      # 24 units of 216 tokens
_row("production-stage1-dropout", S((48, 48, 48), (7, 7, 7), (3, 3, 3), 3, 48, B=1), BF16, win(8), win(8), drop_p=0.1)
_row("production-270-units-dropout", W.PRODUCTION, BF16, win(8), win(8), drop_p=0.25)

# ---- the edges of each predicate
_row("edge-n352", S((352, 1, 1), (352, 1, 1), (0, 0, 0), 1, 16, B=1, tw=8), BF16, win(11), ql(4, 6))
_row("edge-n353", S((353, 1, 1), (353, 1, 1), (0, 0, 0), 1, 16, B=1, tw=8), BF16, ql(4, 6), ql(4, 6))
_row("edge-table-13-cubed", S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16, B=1, tw=7), BF16, win(11), win(8))      # 2197 <= 2200
_row("edge-table-15-cubed", S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16, B=1, tw=8), BF16, win(11), ql(4, 6))      # 3375
_row("edge-units-255", S((102, 2, 2), (2, 2, 2), (0, 0, 0), 5, 80, B=1), BF16, win(11), win(8))      # 51 windows x 5 heads
_row("edge-units-256-unshifted", S((16, 16, 16), (4, 4, 4), (0, 0, 0), 4, 64, B=1), BF16, win(8), win(8))
_row("edge-units-256-unshifted-dropout", S((16, 16, 16), (4, 4, 4), (0, 0, 0), 4, 64, B=1), BF16, win(8), win(8), drop_p=0.25)
_row("edge-head-dim-16-without-a-table", S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16, B=1, table=False), BF16, ql(4, 6), ql(4, 6))
_row("edge-drop-p-below-the-quantum", W.LAYOUT_SPEC, BF16, win(11), win(8), drop_p=1e-9)      # lrintf(p * 65536) == 0: no dropout form
# (1) the query-lane bound refuses a table the window kernels would have to hold too; (6) a 33^3 table passes it at few tokens and does not
# fit behind the forward's tiles, while the backward (fixed slots: query lanes) takes it
_row("edge-table-39-cubed", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 1, 16, B=1, tw=20), BF16, no(UNSUPPORTED, "winattn_fwd: 246940 bytes of LDS needed"),
     no(UNSUPPORTED, "winattn_bwd: 484216 bytes of LDS needed"))
_row("edge-table-33-cubed", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 1, 16, B=1, tw=17), BF16, no(UNSUPPORTED, "winattn_fwd: 182020 bytes of LDS needed"),
     no(UNSUPPORTED, "winattn_bwd: 297160 bytes of LDS needed"))
_row("edge-table-31-cubed", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 1, 16, B=1, tw=16), BF16, win(11), no(UNSUPPORTED, "winattn_bwd: 247992 bytes of LDS needed"))
# (4) an unknown dtype surfaces after the LDS check, (5) drop_p after the geometry
_row("edge-unknown-dtype", W.LAYOUT_SPEC, 7, no(BADARG, "unknown dtype 7"), no(BADARG, "unknown dtype 7"))
_row("edge-unknown-dtype-behind-the-lds-bound", S((7, 7, 7), (7, 7, 7), (0, 0, 0), 2, 128), 7, no(UNSUPPORTED, "bytes of LDS needed"), no(UNSUPPORTED, "bytes of LDS needed"))
_row("edge-drop-p-behind-the-geometry", S((8, 8, 8), (4, 4, 4), (4, 0, 0), 1, 16), BF16, no(BADARG, "shift must be < window"), no(BADARG, "shift must be < window"), drop_p=1.0)
_row("edge-null-qkv", W.LAYOUT_SPEC, BF16, no(BADARG, "winattn: null pointer"), no(BADARG, "winattn: null pointer"), null=("qkv",))
_row("edge-null-dout", W.LAYOUT_SPEC, BF16, win(11), no(BADARG, "winattn_bwd: null pointer"), null=("dout",))

# ---- every refusal of test_refusals_return_before_any_launch, in both dtypes
for _dt, _nm in ((F32, "fp32"), (BF16, "bf16")):
    for _id, _s, _rc, _text, _kw in (
            ("448-tokens", S((8, 8, 7), (8, 8, 7), (0, 0, 0), 1, 16, tw=8), UNSUPPORTED, "max 384 tokens", {}),
            ("shift-4-of-4", S((8, 8, 8), (4, 4, 4), (4, 0, 0), 1, 16), BADARG, "shift must be < window", {}),
            ("shift-5-of-4", S((8, 8, 8), (4, 4, 4), (0, 0, 5), 1, 16), BADARG, "shift must be < window", {}),
            ("table-6-cubed", S((7, 7, 7), (7, 7, 7), (0, 0, 0), 1, 16), BADARG, "smaller than the 343-token window", dict(tw=6)),
            ("head-dim-20", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 2, 40), UNSUPPORTED, "head_dim 20 not instantiated", {}),
            ("head-dim-6", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 2, 12), UNSUPPORTED, "head_dim 6", {}),
            ("head-dim-68", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 2, 136), UNSUPPORTED, "head_dim 68", {}),
            ("drop-p-1", S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48), BADARG, "must lie in [0, 1)", dict(drop_p=1.0)),
            ("drop-p-negative", S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48), BADARG, "must lie in [0, 1)", dict(drop_p=-0.1))):
        _row(f"refusal-{_nm}-{_id}", _s, _dt, no(_rc, _text), no(_rc, _text), **_kw)
    # a table gradient without a table: only the backward refuses
    _row(f"refusal-{_nm}-dtable-without-table", S((6, 6, 6), (6, 6, 6), (0, 0, 0), 3, 48, table=False), _dt, ql(4, 4), no(BADARG, "dbias_table given without a bias_table"),
         dtable="force")
    _row(f"refusal-{_nm}-dtable-without-table-padded", S((9, 5, 6), (4, 4, 4), (2, 2, 2), 2, 32, table=False), _dt, ql(4, 1), no(BADARG, "dbias_table given without a bias_table"),
         dtable="force")
_row("refusal-fp32-head-dim-64-at-343-tokens", S((7, 7, 7), (7, 7, 7), (0, 0, 0), 2, 128), F32, no(UNSUPPORTED, "winattn_fwd: 192032 bytes of LDS needed"),
     no(UNSUPPORTED, "winattn_bwd: 200820 bytes of LDS needed"))
_row("refusal-bf16-global-dtable-without-table", S((4, 4, 4), (4, 4, 4), (0, 0, 0), 1, 64, table=False), BF16, glob(4, 1), no(BADARG, "dbias_table given without a bias_table"),
     dtable="force")

# ---- the instantiations and a row for each (the form the row is there for is its expected plan)
WINDOW_FWD_FORMS = {(m, w, d) for m in (0, 1) for w in (8, 11) for d in (0, 1)}      # <MASK, NW, DROP>
WINDOW_BWD_FORMS = {(m, t, 8, d) for m in (0, 1) for t in (0, 1) for d in (0, 1)}      # <MASK, DT, NW, DROP>
GLOBAL_FORMS = {(t, d) for t in (2, 4, 6, 8, 10, 12, 14, 16) for d in (0, 1)}      # <NT, DROP>, either direction
QUERY_LANE_FORMS = {(dt, h) for dt in (F32, BF16) for h in (1, 2, 3, 4, 8, 16)}      # <T, HD4>, either direction
_SHAPE = {8: ((16, 16, 16), (4, 4, 4), 4), 11: ((6, 6, 6), (6, 6, 6), 3)}      # waves -> (dims, window, heads): 256 units, 3 units
for _m in (0, 1):
    for _wv in (8, 11):
        for _d in (0, 1):
            for _v in (1, 0):
                _dims, _ws, _h = _SHAPE[_wv]
                _s = S(_dims, _ws, (1, 1, 1) if _m else (0, 0, 0), _h, 16 * _h, B=1)
                _row(f"form-window-mask{_m}-waves{_wv}-drop{_d}-vec{_v}", _s, BF16, win(_wv, _v), win(8, _v), drop_p=0.25 * _d, dtable=bool(_d), lay={} if _v else {"qkv": "off8"})
                _row(f"form-window-mask{_m}-waves{_wv}-drop{_d}-vec{_v}-other-dtable", _s, BF16, win(_wv, _v), win(8, _v), drop_p=0.25 * _d, dtable=not _d, lay={} if _v else {"qkv": "off8"})
for _t, _dims in ((2, (1, 4, 8)), (4, (2, 4, 8)), (6, (3, 4, 8)), (8, (4, 4, 8)), (10, (5, 4, 8)), (12, (6, 4, 8)), (14, (7, 4, 8)), (16, (8, 4, 8))):
    for _d in (0, 1):
        _row(f"form-global-tiles{_t}-drop{_d}", _G(_dims, B=2, heads=2), BF16, glob(_t, _t // 4 + (_t % 4 > 0)), glob(_t, 2 * (_t // 4 + (_t % 4 > 0))), drop_p=0.1 * _d)
for _dt, _nm in ((F32, "fp32"), (BF16, "bf16")):
    for _h4 in (1, 2, 3, 4, 8, 16):
        _row(f"form-query-lane-{_nm}-hd4-{_h4}", S((5, 5, 5), (3, 3, 3), (1, 1, 1), 2, 8 * _h4, table=False), _dt, ql(_h4, 1), ql(_h4, 1))


def find(spec, dt, drop_p=0.0, lay=None, dtable=True, dqb=True):
    """(forward, backward) short forms of the row with this spec, dtype and request"""
    want = (spec, dt, float(drop_p), lay or {}, bool(dtable), bool(dqb))
    for _, s, d, kw, fwd, bwd in ROWS:
        if "tw" not in kw and "null" not in kw and (s, d, float(kw.get("drop_p", 0.0)), kw.get("lay") or {}, kw.get("dtable", True), kw.get("dqb", True)) == want:
            return fwd, bwd
    raise KeyError(f"no row for {spec} dtype {dt} p={drop_p} {lay} dtable={dtable} dqb={dqb}")


def launcher_forms():
    """the instantiation lists of the launchers, read from the source: (window forward, window backward, query lanes) of csrc/attention.hip
    and the global kernels' of csrc/attention_global.hip"""
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mi-seg_amd", "csrc")
    val = {"true": 1, "false": 0, "float": F32, "bf16": BF16}

    def forms(src, name):      # the macro's replacement text: its line and the continuation lines behind it
        lines = src[src.index("#define %s(X)" % name):].split("\n")
        n = next(i for i, ln in enumerate(lines) if not ln.rstrip().endswith("\\"))
        body = " ".join(ln.rstrip().rstrip("\\") for ln in lines[:n + 1]).split(")", 1)[1]
        return [tuple(int(val.get(t.strip(), t.strip())) for t in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", body)]

    att = open(os.path.join(here, "attention.hip")).read()
    glb = open(os.path.join(here, "attention_global.hip")).read()
    return forms(att, "WINDOW_FWD_FORMS"), forms(att, "WINDOW_BWD_FORMS"), forms(att, "QUERY_LANE_FORMS"), forms(glb, "GLOBAL_FORMS")


# ================================================================================================ the sweep over the two question entry points
DIMS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 14, 16, 20, 24, 33, 48]
WINDOWS = [7, 4, 2, 3, 6, 7, 1, 5, 4, 8, 11, 22]
HEAD_DIM = [16, 64, 4, 8, 12, 32, 20, 6, 68, 16]
HEADS = [1, 2, 3, 4, 6, 12, 24]
TABLE_WINDOW = [7, 8, 6, 2, 16, 17, 20, 0]
DROP_P = [0.0, 0.25, 1e-9, 0.999, 1.0, -0.1]
OFFSETS = [0, 16, 8, 4, 2]      # bytes
SLACK = [0, 8, 4, 1, 9]      # elements


def sweep(plan_so, so, L, count, seed, each=None):
    """`count` drawn parameter sets: sha256 over (direction, answer) of `so`'s two question entry points on the sets `plan_so`'s plan of that
    direction accepts.  Returns (hex digest, {"accepted": (fwd, bwd), "yes": (fwd, bwd) answered 1 among them, "refused": (fwd, bwd),
    "refused_yes": [(direction, the plan's message, parameters) of every refused set `so` answers 1 for]}).  each(f, b, plans, codes): called per set."""
    import ctypes as C
    state = [seed & (2 ** 64 - 1)]

    def draw(n):      # a 64-bit LCG of our own (Knuth's MMIX constants): the same draws under every Python
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (state[0] >> 33) % n

    def pick(vs, plain=4):      # the first value `plain - 1` times out of `plain`
        return vs[0] if draw(plain) else vs[draw(len(vs))]

    h = hashlib.sha256()
    acc, yes, ref, refused_yes = [0, 0], [0, 0], [0, 0], []
    plf, plb = L.WinattnPlan(), L.WinattnPlan()
    for _ in range(count):
        kind = draw(4)      # 0: a global shape, else windows
        if kind == 0:
            dims = tuple(DIMS[draw(9)] for _ in range(3))
            ws = dims if draw(8) else tuple(WINDOWS[draw(len(WINDOWS))] for _ in range(3))
            hd, table = pick(HEAD_DIM[1:], 6), draw(8) == 0
        else:
            dims = tuple(DIMS[draw(len(DIMS))] for _ in range(3))
            ws = tuple(pick(WINDOWS, 3) for _ in range(3))
            hd, table = pick(HEAD_DIM, 3), draw(8) != 0
        ss = tuple((draw(w) if draw(16) else w) if draw(2) else 0 for w in ws) if draw(3) else (0, 0, 0)
        heads = HEADS[draw(len(HEADS))]
        spec = S(dims, ws, ss, heads, hd * heads, B=1 + draw(3), table=table, bias=bool(draw(4)))
        null = tuple(o for o in OPERANDS + ("lse",) if draw(256) == 0)
        f, b = params(L, spec, dt=pick([BF16, F32, BF16, 7], 2), drop_p=pick(DROP_P, 3), tw=pick(TABLE_WINDOW, 3) if table else pick([1, 7, 0]),
                      dtable="force" if draw(32) == 0 else bool(draw(2)), dqb=bool(draw(2)), null=null,
                      off={o: pick(OFFSETS) for o in OPERANDS}, slack={o: pick(SLACK) for o in OPERANDS})
        codes = (plan_so.miseg_winattn_fwd_plan(C.byref(f), C.byref(plf)), plan_so.miseg_winattn_bwd_plan(C.byref(b), C.byref(plb)))
        msgs = []
        for d, (prm, rc) in enumerate(((f, codes[0]), (b, codes[1]))):      # the plan's message of a refusal, before the next call overwrites it
            msgs.append(None)
            if rc != 0:
                getattr(plan_so, ("miseg_winattn_fwd_plan", "miseg_winattn_bwd_plan")[d])(C.byref(prm), C.byref(L.WinattnPlan()))
                msgs[d] = plan_so.miseg_last_error().decode()
        got = answers(so, f, b)
        for d in (0, 1):
            if codes[d] == 0:
                h.update(struct.pack("<bb", d, got[d]))
                acc[d] += 1
                yes[d] += got[d]
            else:
                ref[d] += 1
                if got[d]:
                    refused_yes.append((d, msgs[d], str(spec)))
        if each is not None:
            each(f, b, (plf, plb), codes, got)
    return h.hexdigest(), dict(accepted=tuple(acc), yes=tuple(yes), refused=tuple(ref), refused_yes=refused_yes)


# the classes of refused calls for which the question entry points used to answer 1: by the plan's message
REFUSED_CLASSES = ("must lie in [0, 1)", "dbias_table given without a bias_table", "bytes of LDS needed")
