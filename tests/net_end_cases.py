"""The case table of the network-end kernels (csrc/net_end.hip: the one- to four-channel stem convolution, the patch embedding, the
output head): one row per launch form, operand layout and loop condition, each with the kernel its plan must name.  Two files run it:
tests/test_net_end_plan_cpu.py through the host-only plans with stand-in addresses, tests/test_hip_net_end_forms.py on the card - the GPU file
runs exactly the rows the CPU file pinned.  No torch here: shapes, layouts, expectations and the ctypes params of a row.

A row: op, id, dtype ("f32" / "bf16"), B, Cin, Cout, dims (D, H, W: the FINE grid of the image for the stem and the patch embedding, the
volume whose product is S for the head), `lay` the layout of the channels-last operand (tests/layouts.py: "contig", "slice", "off8",
"ldodd"; y of a forward, dy of a weight gradient, x of the head), `lay_dx` that of the head's dx, the optional pointers (bias, dbias, ws,
dx, dw: False = NULL), and what the plan must say: k (kernel; head_bwd: kdx, kdw), partial, passes, wrap (items > workgroups x items per
workgroup and trip: the kernel's loop goes round)."""
import ctypes as C

A = 1 << 12            # an aligned stand-in address: the plans read pointers for NULL and alignment only
ES = {"f32": 4, "bf16": 2}


def nvec(dt):
    return 16 // ES[dt]


def layout(c, dt, lay):
    """(element offset of the view's first channel, leading dimension) of a channels-last operand: what layouts.Slot builds"""
    n = nvec(dt)
    cp = -(-c // n) * n
    return {"contig": (0, c), "slice": (n, cp + 3 * n), "off8": (n // 2, cp + 2 * n), "ldodd": (0, cp + n + 1)}[lay]


ROWS = []


def _row(op, name, dt, B, Cin, Cout, dims, lay="contig", **kw):
    r = dict(op=op, id=f"{op}-{name}-{dt}", dt=dt, B=B, Cin=Cin, Cout=Cout, dims=tuple(dims), lay=lay, lay_dx="contig", bias=True, dbias=True, ws=True,
             dx=True, dw=True, partial=0, passes=1, wrap=False)
    r.update(kw)
    assert all(r["id"] != o["id"] for o in ROWS), r["id"]
    ROWS.append(r)


# kernel names as in hip/lib.py (NE_*); resolved when a test runs
# ---------------------------------------------------------------------------------------------------------------- stem forward
for _d in [(1, 1, 1), (3, 3, 3), (4, 4, 16), (5, 6, 18)]:
    _row("stem_fwd", "mfma-%dx%dx%d" % _d, "bf16", 1, 1, 48, _d, k="NE_STEM_FWD_MFMA")
_row("stem_fwd", "mfma-b2-5x9x17", "bf16", 2, 1, 48, (5, 9, 17), k="NE_STEM_FWD_MFMA")
_row("stem_fwd", "mfma-slice", "bf16", 1, 1, 48, (5, 6, 18), "slice", k="NE_STEM_FWD_MFMA")
_row("stem_fwd", "mfma-off8", "bf16", 1, 1, 48, (5, 6, 18), "off8", k="NE_STEM_FWD_MFMA")      # an 8-byte base stays on the matrix cores
_row("stem_fwd", "mfma-wrap-2197-bricks", "bf16", 1, 1, 48, (50, 51, 200), k="NE_STEM_FWD_MFMA", wrap=True)
for _dt in ("f32", "bf16"):
    for _co in (8, 24, 64):
        _row("stem_fwd", f"brick-1to{_co}", _dt, 2 if _co == 24 else 1, 1, _co, (5, 6, 18), k="NE_STEM_FWD_BRICK")
_row("stem_fwd", "brick-slice", "bf16", 1, 1, 24, (3, 3, 3), "slice", k="NE_STEM_FWD_BRICK")      # (an fp32 slice of layouts.Slot has ld % 8 == 4: generic)
_row("stem_fwd", "generic-1to24-slice-ld36", "f32", 1, 1, 24, (3, 3, 3), "slice", k="NE_STEM_FWD_GENERIC")
_row("stem_fwd", "brick-1to48", "f32", 1, 1, 48, (4, 4, 16), k="NE_STEM_FWD_BRICK")
_row("stem_fwd", "brick-1x1x1", "f32", 1, 1, 8, (1, 1, 1), k="NE_STEM_FWD_BRICK")
_row("stem_fwd", "brick-wrap-4624-bricks", "f32", 1, 1, 8, (66, 67, 250), k="NE_STEM_FWD_BRICK", wrap=True)
for _dt in ("f32", "bf16"):
    for _ci in (2, 3, 4):
        _row("stem_fwd", f"generic-cin{_ci}", _dt, 2 if _ci == 3 else 1, _ci, 24, (5, 6, 18), k="NE_STEM_FWD_GENERIC")
    _row("stem_fwd", "generic-1to20", _dt, 1, 1, 20, (5, 6, 18), k="NE_STEM_FWD_GENERIC")
    _row("stem_fwd", "generic-1to6", _dt, 1, 1, 6, (3, 3, 3), k="NE_STEM_FWD_GENERIC")
    _row("stem_fwd", "generic-1to24-ldodd", _dt, 1, 1, 24, (5, 6, 18), "ldodd", k="NE_STEM_FWD_GENERIC")
    _row("stem_fwd", "generic-1to24-off8", _dt, 1, 1, 24, (5, 6, 18), "off8", k="NE_STEM_FWD_GENERIC")
_row("stem_fwd", "generic-1to48-ldodd", "bf16", 1, 1, 48, (5, 6, 18), "ldodd", k="NE_STEM_FWD_GENERIC")      # ldy % 4 != 0 leaves the matrix cores
_row("stem_fwd", "generic-wrap-2113536-voxels", "f32", 1, 2, 4, (129, 128, 128), k="NE_STEM_FWD_GENERIC", wrap=True)

# ---------------------------------------------------------------------------------------------------------------- stem weight gradient
_row("stem_wgrad", "mfma-12wg-atomics", "bf16", 1, 1, 48, (8, 8, 40), k="NE_STEM_WGRAD_MFMA", partial=0)
_row("stem_wgrad", "mfma-18wg-partial", "bf16", 1, 1, 48, (8, 12, 40), k="NE_STEM_WGRAD_MFMA", partial=1)
_row("stem_wgrad", "mfma-18wg-no-workspace", "bf16", 1, 1, 48, (8, 12, 40), k="NE_STEM_WGRAD_MFMA", ws=False, partial=0)
_row("stem_wgrad", "mfma-b2-ragged", "bf16", 2, 1, 48, (5, 6, 18), k="NE_STEM_WGRAD_MFMA", partial=1)      # 2 x 2 x 2 x 2 = 16 bricks
_row("stem_wgrad", "mfma-b2-ragged-atomics", "bf16", 2, 1, 48, (5, 4, 18), k="NE_STEM_WGRAD_MFMA", partial=0)      # 8 bricks
_row("stem_wgrad", "mfma-slice", "bf16", 1, 1, 48, (5, 6, 18), "slice", k="NE_STEM_WGRAD_MFMA", partial=0)
_row("stem_wgrad", "mfma-wrap-648-bricks", "bf16", 1, 1, 48, (33, 32, 130), k="NE_STEM_WGRAD_MFMA", partial=1, wrap=True)
for _dt in ("f32", "bf16"):
    for _co in (8, 24, 56):
        _row("stem_wgrad", f"brick-cout{_co}", _dt, 2 if _co == 24 else 1, 1, _co, (5, 6, 18), k="NE_STEM_WGRAD_BRICK")
    _row("stem_wgrad", "brick-slice", _dt, 1, 1, 24, (3, 3, 3), "slice", k="NE_STEM_WGRAD_BRICK")
_row("stem_wgrad", "brick-cout48", "f32", 1, 1, 48, (8, 12, 40), k="NE_STEM_WGRAD_BRICK")
_row("stem_wgrad", "brick-wrap-648-bricks", "f32", 1, 1, 8, (33, 32, 130), k="NE_STEM_WGRAD_BRICK", wrap=True)
_row("stem_wgrad", "brick-wrap-648-bricks", "bf16", 1, 1, 8, (33, 32, 130), k="NE_STEM_WGRAD_BRICK", wrap=True)
for _dt in ("f32", "bf16"):
    _row("stem_wgrad", "generic-cin2", _dt, 2, 2, 24, (9, 10, 17), k="NE_STEM_WGRAD_GENERIC")      # no axis a multiple of 8
    _row("stem_wgrad", "generic-cin4", _dt, 1, 4, 24, (8, 8, 16), k="NE_STEM_WGRAD_GENERIC")
    _row("stem_wgrad", "generic-cout20", _dt, 1, 1, 20, (5, 6, 18), k="NE_STEM_WGRAD_GENERIC")
    _row("stem_wgrad", "generic-cout64", _dt, 1, 1, 64, (8, 8, 8), k="NE_STEM_WGRAD_GENERIC")
    _row("stem_wgrad", "generic-ldodd", _dt, 1, 1, 24, (5, 6, 18), "ldodd", k="NE_STEM_WGRAD_GENERIC")
    _row("stem_wgrad", "generic-off8", _dt, 1, 1, 24, (5, 6, 18), "off8", k="NE_STEM_WGRAD_GENERIC")
    _row("stem_wgrad", "generic-3x2x5", _dt, 1, 3, 6, (3, 2, 5), k="NE_STEM_WGRAD_GENERIC")      # smaller than one 8^3 brick

# ---------------------------------------------------------------------------------------------------------------- patch embedding forward
for _dt in ("f32", "bf16"):
    for _ci in (1, 2, 4):
        _row("patch_fwd", f"cin{_ci}-to24", _dt, 1, _ci, 24, (8, 10, 12), k="NE_PATCH_FWD")
    _row("patch_fwd", "1to48-b2", _dt, 2, 1, 48, (8, 10, 12), k="NE_PATCH_FWD")
    _row("patch_fwd", "2to20-ragged-group", _dt, 2, 2, 20, (4, 6, 10), k="NE_PATCH_FWD")
    _row("patch_fwd", "no-bias", _dt, 1, 2, 24, (2, 2, 2), k="NE_PATCH_FWD", bias=False)
    _row("patch_fwd", "2x2x2", _dt, 1, 1, 20, (2, 2, 2), k="NE_PATCH_FWD")
    for _lay in ("slice", "off8", "ldodd"):
        _row("patch_fwd", f"1to24-{_lay}", _dt, 1, 1, 24, (4, 6, 10), _lay, k="NE_PATCH_FWD")
_row("patch_fwd", "wrap-2116800-items", "bf16", 1, 1, 48, (144, 140, 140), k="NE_PATCH_FWD", wrap=True)

# ---------------------------------------------------------------------------------------------------------------- patch embedding backward
for _dt in ("f32", "bf16"):
    _six = 24 if _dt == "f32" else 48      # six 16-byte vectors per row: 42 rows per trip, 168 per workgroup
    _row("patch_bwd", f"team-cout{_six}-15wg-atomics", _dt, 1, 1, _six, (24, 28, 30), k="NE_PATCH_BWD_TEAM", partial=0)
    _row("patch_bwd", f"team-cout{_six}-16wg-partial", _dt, 1, 1, _six, (26, 28, 28), k="NE_PATCH_BWD_TEAM", partial=1)
    _row("patch_bwd", f"team-cout{_six}-16wg-no-workspace", _dt, 1, 1, _six, (26, 28, 28), k="NE_PATCH_BWD_TEAM", ws=False, partial=0)
    _row("patch_bwd", f"team-cout{_six}-cin2-partial", _dt, 1, 2, _six, (26, 28, 28), k="NE_PATCH_BWD_TEAM", partial=1)
    _row("patch_bwd", f"team-cout{72 - _six}-cin4", _dt, 1, 4, 72 - _six, (8, 10, 12), k="NE_PATCH_BWD_TEAM", partial=0)
    _row("patch_bwd", "team-cin2-no-dbias", _dt, 1, 2, 24, (8, 10, 12), k="NE_PATCH_BWD_TEAM", dbias=False, partial=0)
    _row("patch_bwd", "team-cin2-partial-no-dbias", _dt, 1, 2, _six, (26, 28, 28), k="NE_PATCH_BWD_TEAM", dbias=False, partial=1)
    _row("patch_bwd", "team-b2-slice", _dt, 2, 2, 24, (4, 6, 10), "slice", k="NE_PATCH_BWD_TEAM", partial=0)
    _rag = 22 if _dt == "f32" else 20      # no whole number of 16-byte vectors
    _row("patch_bwd", f"generic-cout{_rag}", _dt, 2, 1, _rag, (6, 10, 14), k="NE_PATCH_BWD_GENERIC")      # 210 coarse voxels: the last block of 64 holds 18
    _row("patch_bwd", "generic-cout24-ldodd", _dt, 1, 1, 24, (4, 6, 10), "ldodd", k="NE_PATCH_BWD_GENERIC")
    _row("patch_bwd", "generic-cout24-off8", _dt, 1, 2, 24, (4, 6, 10), "off8", k="NE_PATCH_BWD_GENERIC")
    _row("patch_bwd", "generic-cin4-no-dbias", _dt, 1, 4, _rag, (6, 10, 14), k="NE_PATCH_BWD_GENERIC", dbias=False)
    _row("patch_bwd", "generic-cin4-3blocks", _dt, 1, 4, _rag, (24, 28, 30), k="NE_PATCH_BWD_GENERIC")      # 2520 coarse voxels, three workgroups

# ---------------------------------------------------------------------------------------------------------------- head forward
for _dt in ("f32", "bf16"):
    for _co in (1, 2, 6, 9, 16):
        _row("head_fwd", f"tile-48to{_co}", _dt, 1, 48, _co, (5, 6, 7), k="NE_HEAD_FWD_TILE")
    _row("head_fwd", "tile-96to6-no-bias", _dt, 1, 96, 6, (5, 6, 7), k="NE_HEAD_FWD_TILE", bias=False)
    _row("head_fwd", "tile-slice", _dt, 1, 48, 6, (5, 6, 7), "slice", k="NE_HEAD_FWD_TILE")
    _row("head_fwd", "tile-b2-s210", _dt, 2, 48, 6, (5, 6, 7), k="NE_HEAD_FWD_TILE")      # a 256-voxel tile straddles the two samples
    _row("head_fwd", "tile-s1", _dt, 1, 48, 6, (1, 1, 1), k="NE_HEAD_FWD_TILE")
    _row("head_fwd", "scalar-6to6", _dt, 2, 6, 6, (5, 6, 7), k="NE_HEAD_FWD_SCALAR")
    _row("head_fwd", "scalar-50to9", _dt, 1, 50, 9, (5, 6, 7), k="NE_HEAD_FWD_SCALAR")
    _row("head_fwd", "scalar-48-ldodd", _dt, 1, 48, 6, (5, 6, 7), "ldodd", k="NE_HEAD_FWD_SCALAR")
    _row("head_fwd", "scalar-48-off8", _dt, 1, 48, 6, (5, 6, 7), "off8", k="NE_HEAD_FWD_SCALAR")
_row("head_fwd", "tile-wrap-1175-tiles", "bf16", 1, 48, 2, (67, 67, 67), k="NE_HEAD_FWD_TILE", wrap=True)
_row("head_fwd", "scalar-wrap-2113536-voxels", "bf16", 1, 6, 1, (129, 128, 128), k="NE_HEAD_FWD_SCALAR", wrap=True)

# ---------------------------------------------------------------------------------------------------------------- head backward (dx and dw)
for _co in (1, 6, 8):
    _row("head_bwd", f"dxtile-dwmfma-48to{_co}", "bf16", 1, 48, _co, (4, 8, 8), kdx="NE_HEAD_DX_TILE", kdw="NE_HEAD_DW_MFMA")
_row("head_bwd", "dxtile-dwmfma-b2-s512", "bf16", 2, 48, 6, (8, 8, 8), kdx="NE_HEAD_DX_TILE", kdw="NE_HEAD_DW_MFMA")
_row("head_bwd", "dxtile-dwmfma-dx-slice", "bf16", 2, 48, 6, (4, 8, 8), kdx="NE_HEAD_DX_TILE", kdw="NE_HEAD_DW_MFMA", lay_dx="slice")
_row("head_bwd", "dxtile-dwteam-256to2", "bf16", 1, 256, 2, (4, 8, 8), kdx="NE_HEAD_DX_TILE", kdw="NE_HEAD_DW_TEAM")      # 32 vectors per row
_row("head_bwd", "dxtile-dwteam-96to6", "bf16", 2, 96, 6, (4, 8, 8), kdx="NE_HEAD_DX_TILE", kdw="NE_HEAD_DW_TEAM")
_row("head_bwd", "dxtile-dwmfma-wrap-1168-tiles", "bf16", 1, 48, 2, (73, 64, 64), kdx="NE_HEAD_DX_TILE", kdw="NE_HEAD_DW_MFMA", wrap=True)
_row("head_bwd", "dxteam-dwmfma-48to16", "bf16", 2, 48, 16, (4, 8, 8), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_MFMA")
_row("head_bwd", "dxteam-dwmfma-48to9", "bf16", 1, 48, 9, (4, 8, 8), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_MFMA")
_row("head_bwd", "dxteam-dwteam-s210", "bf16", 2, 48, 6, (5, 6, 7), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM")
_row("head_bwd", "dxteam-dwteam-s210-48to9", "bf16", 2, 48, 9, (5, 6, 7), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM", passes=2)
_row("head_bwd", "dxteam-dwteam-s210-48to16", "bf16", 1, 48, 16, (5, 6, 7), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM", passes=2)
for _co, _ps in ((1, 1), (6, 1), (9, 2), (16, 2)):
    _row("head_bwd", f"dxteam-dwteam-48to{_co}", "f32", 2, 48, _co, (4, 8, 8), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM", passes=_ps)
_row("head_bwd", "dxteam-dwteam-s210", "f32", 2, 48, 6, (5, 6, 7), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM")
_row("head_bwd", "dxteam-dwteam-96to9-slices", "f32", 1, 96, 9, (5, 6, 7), "slice", kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM", passes=2, lay_dx="slice")
_row("head_bwd", "dxteam-wrap-2107392-items", "f32", 1, 48, 2, (56, 56, 56), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM", wrap=True)
for _dt in ("f32", "bf16"):
    _row("head_bwd", "dwteam-3-rows", _dt, 1, 48, 6, (1, 1, 3), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM")      # fewer rows than one round of the team
    _row("head_bwd", "scalar-6to6", _dt, 2, 6, 6, (5, 6, 7), kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC")
    _row("head_bwd", "scalar-50to9", _dt, 1, 50, 9, (5, 6, 7), kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC")
    _row("head_bwd", "scalar-48-ldodd", _dt, 1, 48, 6, (5, 6, 7), "ldodd", kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC", lay_dx="ldodd")
    _row("head_bwd", "scalar-48-off8", _dt, 1, 48, 6, (5, 6, 7), "off8", kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC", lay_dx="off8")
    _row("head_bwd", "scalar-16-blocks-of-64", _dt, 1, 6, 2, (3, 31, 32), kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC")      # 2976 voxels, two workgroups of the weight gradient
    _row("head_bwd", "no-dx", _dt, 2, 48, 6, (5, 6, 7), kdx="NE_NONE", kdw="NE_HEAD_DW_TEAM", dx=False)
    _row("head_bwd", "no-dw", _dt, 2, 48, 6, (5, 6, 7), kdx="NE_HEAD_DX_TEAM", kdw="NE_NONE", dw=False, dbias=False)
    _row("head_bwd", "no-dbias", _dt, 2, 48, 9, (5, 6, 7), kdx="NE_HEAD_DX_TEAM", kdw="NE_HEAD_DW_TEAM", dbias=False, passes=2)
    _row("head_bwd", "scalar-no-dbias", _dt, 1, 50, 6, (5, 6, 7), kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC", dbias=False)
_row("head_bwd", "mfma-no-dx-no-dbias", "bf16", 2, 48, 6, (4, 8, 8), kdx="NE_NONE", kdw="NE_HEAD_DW_MFMA", dx=False, dbias=False)
_row("head_bwd", "scalar-wrap-2113536-voxels", "f32", 1, 6, 1, (129, 128, 128), kdx="NE_HEAD_DX_SCALAR", kdw="NE_HEAD_DW_GENERIC", wrap=True)

PLAN_FN = {"stem_fwd": "miseg_conv3_thin_fwd_plan", "stem_wgrad": "miseg_conv3_thin_wgrad_plan", "patch_fwd": "miseg_patch_embed_fwd_plan",
           "patch_bwd": "miseg_patch_embed_bwd_plan", "head_fwd": "miseg_head_fwd_plan", "head_bwd": "miseg_head_bwd_plan"}
CALL_FN = {op: fn[:-len("_plan")] for op, fn in PLAN_FN.items()}


def S_of(r):
    return r["dims"][0] * r["dims"][1] * r["dims"][2]


def standins(r):
    """stand-in addresses of a row's operands: aligned, or 8 bytes into a 16-byte unit for "off8"; 0 where the row leaves a pointer NULL"""
    off, _ = layout(r["Cin"] if r["op"].startswith("head") else r["Cout"], r["dt"], r["lay"])
    a = {"x": A, "w": A, "y": A, "dy": A, "dw": A if r["dw"] else 0, "bias": A if r["bias"] else 0, "dbias": A if r["dbias"] else 0,
         "ws": A if r["ws"] else 0, "dx": 0}
    rows_op = {"stem_fwd": "y", "patch_fwd": "y", "stem_wgrad": "dy", "patch_bwd": "dy", "head_fwd": "x", "head_bwd": "x"}[r["op"]]
    a[rows_op] = A + off * ES[r["dt"]]
    if r["op"] == "head_bwd" and r["dx"]:
        a["dx"] = A + layout(r["Cin"], r["dt"], r["lay_dx"])[0] * ES[r["dt"]]
    return a


def params(r, L, a):
    """the ctypes params struct of a row's call with the addresses `a` (standins(r), or those of real tensors)"""
    dt = L.BF16 if r["dt"] == "bf16" else L.F32
    B, Cin, Cout, (D, H, W) = r["B"], r["Cin"], r["Cout"], r["dims"]
    op = r["op"]
    if op.startswith("head"):
        ldx = layout(Cin, r["dt"], r["lay"])[1]
        if op == "head_fwd":
            return L.Head(a["x"], ldx, a["y"], a["w"], a["bias"], B, D * H * W, Cin, Cout, dt)
        lddx = layout(Cin, r["dt"], r["lay_dx"])[1] if r["dx"] else 0
        return L.HeadBwd(a["x"], ldx, a["dy"], a["dx"], lddx, a["w"], a["dw"], a["dbias"], B, D * H * W, Cin, Cout, dt)
    ld = layout(Cout, r["dt"], r["lay"])[1]
    if op == "stem_fwd":
        return L.Conv3Thin(a["x"], a["y"], ld, a["w"], B, Cin, D, H, W, Cout, dt)
    if op == "stem_wgrad":
        return L.Conv3ThinWgrad(a["x"], a["dy"], ld, a["dw"], B, Cin, D, H, W, Cout, dt, a["ws"])
    if op == "patch_fwd":
        return L.PatchEmbed(a["x"], a["y"], ld, a["w"], a["bias"], B, Cin, D, H, W, Cout, dt)
    return L.PatchEmbedBwd(a["x"], a["dy"], ld, a["dw"], a["dbias"], B, Cin, D, H, W, Cout, dt, a["ws"])


def plan(r, L, prm):
    """(return code, plan struct) of the row's plan call on `prm`"""
    pl = L.HeadBwdPlan() if r["op"] == "head_bwd" else L.NetEndLaunch()
    return getattr(L.load(), PLAN_FN[r["op"]])(C.byref(prm), C.byref(pl)), pl


def launches(r, pl):
    """[(what, launch entry, expected kernel name)] of a row's plan"""
    if r["op"] == "head_bwd":
        return [("dx", pl.dx, r["kdx"]), ("dw", pl.dw, r["kdw"])]
    return [("", pl, r["k"])]


def wraps(e):
    return e.items > e.workgroups * e.per_workgroup


def check_plan(r, L, rc, pl):
    """the plan names the form the row is there for: kernel, partial-sum route, passes, 32-bit items, and a wrapping loop where the row says so"""
    assert rc == 0, (r["id"], rc, L.load().miseg_last_error())
    for what, e, kname in launches(r, pl):
        assert e.kernel == getattr(L, kname), f"{r['id']} {what}: plan names kernel {e.kernel}, the row is there for {kname} = {getattr(L, kname)}"
        if e.kernel == L.NE_NONE:
            assert (e.workgroups, e.passes, e.items) == (0, 0, 0), r["id"]
            continue
        assert e.workgroups >= 1 and e.per_workgroup >= 1 and e.items >= 1, r["id"]
        assert e.workgroups_y == (r["Cin"] if e.kernel == L.NE_PATCH_BWD_TEAM else 1), r["id"]
        assert e.passes == (r["passes"] if e.kernel == L.NE_HEAD_DW_TEAM else 1), f"{r['id']} {what}: {e.passes} passes"
        assert e.partial == (r["partial"] if e.kernel in (L.NE_STEM_WGRAD_MFMA, L.NE_PATCH_BWD_TEAM) else 0), f"{r['id']} {what}: partial {e.partial}"
        assert e.idx32 == (1 if e.kernel in (L.NE_PATCH_FWD, L.NE_HEAD_DX_TEAM) else 0), f"{r['id']} {what}: idx32 {e.idx32}"      # every test-sized problem
    if r["wrap"]:
        assert any(wraps(e) for _, e, _ in launches(r, pl) if e.kernel != L.NE_NONE), f"{r['id']}: no loop of this row wraps"
