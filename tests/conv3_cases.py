"""The case table of the 3x3x3 weight-gradient kernels (csrc/conv3d.hip: miseg_conv3_wgrad, miseg_conv3_wgrad_group) and of the weight packs: one
row per launch form, volume edge and operand layout, each with the form the library must answer for it (miseg_conv3_wgrad_form /
miseg_conv3_wgrad_group_form - what the launchers dispatch on).  Two files run it: tests/test_conv3_forms_cpu.py through the host-only form
calls with stand-in addresses, tests/test_hip_conv3_forms.py on the card - the GPU file launches exactly the rows the CPU file pinned.  No
torch here: shapes, layouts, expectations and the ctypes params of a row.

A weight-gradient row (WGRAD): id, dt ("f32" / "bf16"), B, dims (D, H, W), Cin, Cout, the layouts of x and dy (tests/layouts.py: "contig",
"slice", "off8", "ldodd"), accumulate, max_workgroups (cap) and `form`: what the row is there for - the kernel, the loop (pipelined or not, one
brick per workgroup or a walk), the route (direct epilogue in its mode, or slabs with one or several splits per reduce group, atomic or not),
the narrow kernel's <NCO, NCI>, the tiny kernel's <S>.  The id is BUILT from these fields, so an id cannot promise another form than the CPU
test pins.  A grouped row (GROUP) holds its layers, the cap of descs[0], per layer (nsplit, direct, piped) and the (PIPED, WALK) grids of the
launch."""
import ctypes as C

A = 1 << 12            # an aligned stand-in address: the form calls read pointers for NULL and alignment only
ES = {"f32": 4, "bf16": 2}
UNSUPPORTED = -2       # MISEG_E_UNSUPPORTED


def nvec(dt):
    return 16 // ES[dt]


def layout(c, dt, lay):
    """(element offset of the view's first channel, leading dimension) of a channels-last operand: what layouts.Slot builds"""
    n = nvec(dt)
    cp = -(-c // n) * n
    return {"contig": (0, c), "slice": (n, cp + 3 * n), "off8": (n // 2, cp + 2 * n), "ldodd": (0, cp + n + 1)}[lay]


WGRAD, GROUP = [], []


# ================================================================================================================ weight gradient
def _wg_id(f, name, dt, acc):
    k = f["kernel"]
    if k == "NARROW":
        return f"narrow-{f['narrow_nco']}x{f['narrow_nci']}" + ("-cap" if f.get("cap") else "") + ("-walk" if f.get("walk") else "") + f"-mode{acc}-{name}"
    if k == "TINY":
        return f"wtiny-s{f['tiny_s']}-mode{acc}-{name}"
    route = f"direct{f['direct']}" if f["direct"] else ("slabs-spg1" if f["spg"] == 1 else "slabs-spgN") + ("-atomic" if f["atomic"] else "")
    return f"wgrad-{dt}-{'piped' if f['piped'] else 'plain'}-{'walk' if f['walk'] else 'one'}-{route}-{name}"


def wgrad(name, dt, B, dims, Cin, Cout, form, acc=0, cap=0, x="contig", dy="contig"):
    f = dict(form)
    r = dict(call="wgrad", dt=dt, B=B, dims=tuple(dims), Cin=Cin, Cout=Cout, form=f, acc=acc, cap=cap, lay=dict(x=x, dy=dy))
    r["id"] = _wg_id(f, name, dt, acc)
    assert all(r["id"] != o["id"] for o in WGRAD), r["id"]
    WGRAD.append(r)


def slab(piped, walk, direct, spg=0, atomic=0, **more):
    """direct: 0 = slab route (spg: 1 or "N" = more than one split per reduce group; atomic: more than one group), else the mode the epilogue runs in"""
    return dict(kernel="SLAB", piped=piped, walk=walk, direct=direct, spg=spg, atomic=atomic, **more)


# the loop that is not pipelined: fp32 always; bf16 with ragged channels, misaligned operands, or a volume thinner than one brick along an axis
for _acc in (0, 1, 2):
    wgrad(f"one-brick-mode{_acc}", "f32", 1, (2, 8, 8), 48, 48, slab(0, 0, 1 if _acc == 1 else 2), acc=_acc)
    wgrad(f"one-brick-d3-mode{_acc}", "bf16", 1, (3, 8, 8), 48, 48, slab(0, 0, 1 if _acc == 1 else 2), acc=_acc)
    wgrad(f"mode{_acc}", "f32", 1, (5, 9, 11), 24, 48, slab(0, 0, 0, 1, 1), acc=_acc)                      # 3 x 2 x 2 = 12 bricks, 12 slabs
    wgrad(f"mode{_acc}", "bf16", 1, (5, 9, 11), 40, 72, slab(0, 0, 0, 1, 1), acc=_acc)                     # ragged channels (40 -> 72): 8 bricks
    wgrad(f"256-bricks-mode{_acc}", "f32", 1, (9, 63, 127), 48, 48, slab(0, 1, 0, "N", 1), acc=_acc)        # 5 x 8 x 16 = 640 bricks over 256 workgroups
wgrad("h7", "bf16", 1, (4, 7, 8), 48, 48, slab(0, 0, 2))
wgrad("w5-b2", "bf16", 2, (9, 9, 5), 48, 96, slab(0, 0, 0, 1, 1))
wgrad("x-off8", "bf16", 1, (5, 9, 11), 48, 48, slab(0, 0, 0, 1, 1, vec_x=0), x="off8")
wgrad("dy-ldodd", "bf16", 1, (5, 9, 11), 48, 48, slab(0, 0, 0, 1, 1, vec_dy=0), dy="ldodd")
wgrad("slices", "bf16", 1, (5, 9, 11), 48, 48, slab(1, 0, 0, 1, 1), x="slice", dy="slice")                 # aligned slices stay pipelined
wgrad("two-blocks-a-side", "f32", 2, (5, 9, 11), 96, 72, slab(0, 0, 0, "N", 1))
wgrad("two-blocks-a-side", "bf16", 1, (5, 9, 11), 56, 96, slab(0, 0, 0, 1, 1))
wgrad("x-ldodd-dy-off8", "f32", 1, (5, 9, 11), 24, 40, slab(0, 0, 0, 1, 1, vec_x=0, vec_dy=0), x="ldodd", dy="off8")
for _cap in (1, 2, 3):
    wgrad(f"cap{_cap}", "f32", 1, (5, 9, 11), 24, 48, slab(0, 1, *((2,) if _cap == 1 else (0, 1, 1))), cap=_cap)
    wgrad(f"cap{_cap}-d3", "bf16", 2, (3, 9, 11), 48, 40, slab(0, 1, *((1,) if _cap == 1 else (0, 1, 1))), acc=1, cap=_cap)
    wgrad(f"cap{_cap}", "bf16", 1, (5, 9, 19), 48, 48, slab(1, 1, *((2,) if _cap == 1 else (0, 1, 1))), acc=2, cap=_cap)
wgrad("256-bricks", "bf16", 1, (17, 63, 63), 40, 48, slab(0, 1, 0, "N", 1), acc=1)                          # 5 x 8 x 8 = 320 bricks
# the narrow kernels: all four <NCO, NCI>, a cap, more bricks than workgroups, strided operands, a misaligned pair that leaves
for _co, _ci in ((16, 16), (16, 32), (32, 16), (32, 32)):
    wgrad(f"{_ci}to{_co}", "bf16", 2 if _co == _ci else 1, (5, 9, 11), _ci, _co, dict(kernel="NARROW", narrow_nco=_co // 16, narrow_nci=_ci // 16), acc=(_co + _ci) // 16 % 3)
    wgrad(f"{_ci}to{_co}", "bf16", 1, (5, 9, 19), _ci, _co, dict(kernel="NARROW", narrow_nco=_co // 16, narrow_nci=_ci // 16, cap=1, walk=1), acc=_co // 32, cap=5)
wgrad("slices", "bf16", 1, (5, 9, 11), 16, 32, dict(kernel="NARROW", narrow_nco=2, narrow_nci=1), x="slice", dy="slice")
wgrad("cap1-one-workgroup", "bf16", 1, (5, 9, 11), 32, 32, dict(kernel="NARROW", narrow_nco=2, narrow_nci=2, cap=1, walk=1), acc=1, cap=1)
wgrad("not-narrow-x-off8", "bf16", 1, (5, 9, 11), 16, 32, slab(0, 0, 0, 1, 1, vec_x=0), x="off8")
wgrad("not-narrow-dy-ldodd", "bf16", 1, (5, 9, 11), 32, 32, slab(0, 0, 0, 1, 1, vec_dy=0), dy="ldodd")
# the tiny kernels: B = 64 is the last batch they take
for _s in (3, 6):
    wgrad("b64", "bf16", 64, (_s,) * 3, 16, 48, dict(kernel="TINY", tiny_s=_s), acc=0)
    wgrad("b2-slices", "bf16", 2, (_s,) * 3, 32, 96, dict(kernel="TINY", tiny_s=_s), acc=1, x="slice", dy="slice")
    wgrad("b1", "bf16", 1, (_s,) * 3, 48, 48, dict(kernel="TINY", tiny_s=_s), acc=2)
    wgrad(f"not-tiny-b65-{_s}x{_s}x{_s}", "bf16", 65, (_s,) * 3, 16, 48, slab(0, 0, 0, "N", 1))
wgrad("not-tiny-3x3x4", "bf16", 1, (3, 3, 4), 48, 48, slab(0, 0, 2))
wgrad("not-tiny-x-off8", "bf16", 1, (3, 3, 3), 48, 48, slab(0, 0, 2, vec_x=0), x="off8")


def wgrad_standins(r):
    es = ES[r["dt"]]
    return dict(x=A + layout(r["Cin"], r["dt"], r["lay"]["x"])[0] * es, dy=A + layout(r["Cout"], r["dt"], r["lay"]["dy"])[0] * es, dw=A, ws=A)


def wgrad_params(r, L, a):
    B, (D, H, W) = r["B"], r["dims"]
    return L.Conv3Wgrad(a["x"], layout(r["Cin"], r["dt"], r["lay"]["x"])[1], a["dy"], layout(r["Cout"], r["dt"], r["lay"]["dy"])[1], a["dw"], B, D, H, W, r["Cin"],
                        r["Cout"], L.BF16 if r["dt"] == "bf16" else L.F32, r["acc"], a["ws"], r["cap"])


def wgrad_form(L, prm):
    f = L.Conv3WgradForm()
    return L.load().miseg_conv3_wgrad_form(C.byref(prm), C.byref(f)), f


def check_wgrad_form(r, L, rc, f):
    assert rc == 0, (r["id"], rc, L.load().miseg_last_error())
    w = r["form"]
    slabk = L.CONV3_WGRAD_BF16 if r["dt"] == "bf16" else L.CONV3_WGRAD_F32
    kernel = {"SLAB": slabk, "NARROW": L.CONV3_WGRAD_NARROW, "TINY": L.CONV3_WGRAD_TINY}[w["kernel"]]
    assert f.plan.kernel == kernel, f"{r['id']}: the form names kernel {f.plan.kernel}, the row is there for {kernel}"
    if w["kernel"] == "SLAB":
        assert f.brick_depth == (4 if r["dt"] == "bf16" else 2)
        got = dict(piped=f.piped, walk=int(f.bricks_per_workgroup > 1), direct=f.direct, vec_x=f.vec_x, vec_dy=f.vec_dy,
                   spg=0 if f.direct else (1 if f.spg == 1 else "N"), atomic=int(f.reduce_groups > 1))
        want = dict(vec_x=1, vec_dy=1)
        want.update({k: v for k, v in w.items() if k != "kernel"})
        assert got == want, f"{r['id']}: the form says {got} (nsplit {f.nsplit}, {f.nbricks} bricks, spg {f.spg}), the row is there for {want}"
        assert f.fill == int(not f.direct and r["acc"] == 0) and f.workgroups == f.ncob * f.ncib * f.nsplit, r["id"]
        assert f.plan.workspace_bytes == f.workgroups * 27 * 48 * 48 * 4, r["id"]
    elif w["kernel"] == "NARROW":
        assert (f.narrow_nco, f.narrow_nci) == (w["narrow_nco"], w["narrow_nci"]), r["id"]
        assert int(f.bricks_per_workgroup > 1) == w.get("walk", 0) and (f.workgroups == r["cap"]) == bool(w.get("cap")), (r["id"], f.workgroups, f.nbricks)
        assert f.plan.workspace_bytes == f.workgroups * 27 * r["Cin"] * r["Cout"] * 4, r["id"]
    else:
        assert f.tiny_s == w["tiny_s"] and f.plan.workspace_bytes == 0, r["id"]


# ================================================================================================================ grouped launch
def group(name, dt, layers, cap, wants, grids):
    """layers: (B, dims, Cin, Cout, accumulate, layout of x, layout of dy); wants: per layer (nsplit, direct, piped) - the target, and with it
    the splits, follows from the whole group and its cap; grids: the (PIPED, WALK) forms the launch makes"""
    assert len(layers) == len(wants)
    r = dict(call="group", id=f"group-{name}-{dt}", dt=dt, cap=cap, grids=frozenset(grids),
             layers=[dict(B=b, dims=d, Cin=ci, Cout=co, acc=acc, cap=0, dt=dt, lay=dict(x=lx, dy=ldy), want=want) for (b, d, ci, co, acc, lx, ldy), want in zip(layers, wants)])
    r["layers"][0]["cap"] = cap
    GROUP.append(r)


_PLAIN = [(1, (3, 9, 11), 48, 48, 1, "contig", "contig"),       # thinner than a brick: 4 bricks
          (1, (5, 9, 11), 40, 72, 0, "contig", "contig"),       # ragged channels, two blocks on the output side: 8 bricks
          (1, (3, 3, 3), 40, 72, 2, "slice", "contig"),         # one brick: not counted by the target
          (2, (4, 8, 8), 48, 48, 1, "off8", "contig"),          # two bricks: not counted either
          (1, (9, 17, 17), 48, 40, 2, "contig", "ldodd")]       # 27 bricks
_PIPED = [(1, (9, 13, 19), 48, 96, 1, "contig", "contig"),      # 18 bricks
          (2, (4, 8, 8), 48, 48, 2, "slice", "slice"),
          (1, (8, 16, 16), 96, 48, 0, "contig", "contig")]
group("plain", "bf16", _PLAIN, 0, [(1, 1, 0), (2, 0, 0), (1, 2, 0), (1, 1, 0), (4, 0, 0)], {(0, 0)})
group("plain-walk", "bf16", _PLAIN, 3, [(1, 1, 0), (1, 2, 0), (1, 2, 0), (1, 1, 0), (2, 0, 0)], {(0, 1)})
group("mixed", "bf16", _PLAIN[:3] + _PIPED, 0, [(1, 1, 0), (2, 0, 0), (1, 2, 0), (3, 0, 1), (1, 2, 1), (2, 0, 1)], {(0, 0), (1, 0)})
group("mixed-walk", "bf16", _PLAIN[:3] + _PIPED, 4, [(1, 1, 0), (1, 2, 0), (1, 2, 0), (2, 0, 1), (1, 2, 1), (1, 2, 1)], {(0, 1), (1, 1)})
_F32 = [(1, (2, 9, 11), 24, 48, 1, "contig", "contig"), (1, (5, 9, 11), 20, 24, 0, "slice", "ldodd"), (1, (2, 8, 8), 48, 48, 2, "contig", "contig")]
group("plain", "f32", _F32, 0, [(1, 1, 0), (2, 0, 0), (1, 2, 0)], {(0, 0)})
group("plain-walk", "f32", _F32, 2, [(1, 1, 0), (2, 0, 0), (1, 2, 0)], {(0, 1)})


def group_params(r, L, addrs):
    """the descriptor array of a grouped row; addrs[i] = dict(x, dy, dw) of layer i (wgrad_standins, or real tensors)"""
    descs = (L.Conv3Wgrad * len(r["layers"]))()
    for i, (l, a) in enumerate(zip(r["layers"], addrs)):
        descs[i] = wgrad_params(l, L, dict(a, ws=0))
    return descs


def group_form(r, L, descs):
    forms = (L.Conv3WgradForm * len(r["layers"]))()
    return L.load().miseg_conv3_wgrad_group_form(descs, len(r["layers"]), forms), forms


def check_group_form(r, L, rc, forms):
    assert rc == 0, (r["id"], rc, L.load().miseg_last_error())
    for i, (l, f) in enumerate(zip(r["layers"], forms)):
        assert (f.nsplit, f.direct, f.piped) == l["want"], f"{r['id']} layer {i}: (nsplit, direct, piped) = {(f.nsplit, f.direct, f.piped)}, the row says {l['want']}"
    assert {(f.piped, f.walk) for f in forms} == r["grids"], (r["id"], {(f.piped, f.walk) for f in forms})


# ================================================================================================================ packs
# (layer Cin, layer Cout, dtype): every layout class of miseg_pack_conv3_weight on either side - K rows of whole 96-byte chunks, of four and of
# two 16-byte groups (bf16), rows padded to the next chunk, rows the row-major kernel serves, ragged channel counts on the N side
PACK_SHAPES = [(48, 48, "bf16"), (96, 40, "bf16"), (32, 72, "bf16"), (64, 32, "bf16"), (16, 24, "bf16"), (16, 16, "bf16"), (40, 16, "bf16"), (130, 24, "bf16"),
               (100, 48, "bf16"), (8, 12, "bf16"), (24, 96, "bf16"), (5, 130, "bf16"), (144, 48, "bf16"), (192, 96, "bf16"),
               (24, 24, "f32"), (48, 72, "f32"), (20, 16, "f32"), (28, 24, "f32"), (12, 40, "f32"), (96, 12, "f32"), (5, 7, "f32")]
