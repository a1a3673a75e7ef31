"""The case table of the 3x3x3 forward / data-gradient launch (csrc/conv3d.hip: miseg_conv3_fwd): one row per launch form, epilogue piece, volume
edge and operand layout, each with the form the library must answer for it (miseg_conv3_fwd_form - the struct conv3_fwd_launch dispatches on).
Two files run it: tests/test_conv3_fwd_forms_cpu.py through the host-only form call with stand-in addresses, tests/test_hip_conv3_fwd_forms.py on
the card - the GPU file launches exactly the rows the CPU file pinned.  No torch here: shapes, layouts, expectations and the ctypes params.

A row: id, dt ("f32" / "bf16"), B, dims (D, H, W), Cin -> Cout of the LAUNCH (a data-gradient row, dgrad = 1, runs the mirrored pack of the
layer Cout -> Cin on dy), the layouts of x and y (tests/layouts.py), the pieces - res (a layout or None), stat, sc = (sc_C, layout of sc_x),
s2c = s2c_C, fs = (fs_stat, layout of fs_y), bg (background), defer (defer_slabs), `refuse`: the pieces the launch must refuse with
MISEG_E_UNSUPPORTED - and `form`: what the row is there for - the kernel ("F96": conv3_fwd96_kernel<T, nt, wd, epi, gpt>, "TINY":
conv3_fwd_tiny_kernel<mt, mg>, "RM": the row-major conv3_fwd_kernel<T, nt>), nt, gpt, splits, chunks per split, epi, vec_x / vec_y / vec_r.
The id is BUILT from these fields, so an id cannot promise another form than the CPU test pins."""
import ctypes as C

from conv3_cases import A, ES, UNSUPPORTED, layout, nvec      # noqa: F401  (one layout rule, one stand-in address for both conv tables)

FWD = []
MAX_ROWS = 160
PIECES = ("res", "stat", "sc", "s2c", "fs")


def cdiv(a, b):
    return -(-a // b)


def vec_of(c, dt, lay):
    """1: an operand of c channels in this layout has a 16-byte aligned base and whole vectors per row (0 without the operand)"""
    return int(lay == "slice" or (lay == "contig" and c % nvec(dt) == 0))


def F96(nt, gpt=6, epi=0, splits=1, cps=1, **vec):
    return dict(kernel="F96", nt=nt, gpt=gpt, epi=epi, splits=splits, cps=cps, **vec)


def TINY(mt, mg, splits, nt):
    return dict(kernel="TINY", tiny=(mt, mg), splits=splits, cps=1, gpt=6, nt=nt, epi=0)


def RM(nt, **vec):
    return dict(kernel="RM", nt=nt, gpt=0, epi=0, splits=1, cps=0, **vec)


def _id(r):
    f, dt = r["form"], r["dt"]
    vec = "".join(f"-{k.replace('vec_', 'v')}0" for k in ("vec_x", "vec_y", "vec_r") if f.get(k) == 0 and (k != "vec_r" or r["res"]))
    if f["kernel"] == "TINY":
        head = f"tiny-{f['tiny'][0]}x{f['tiny'][1]}-s{f['splits']}"
    elif f["kernel"] == "RM":
        head = f"rm-{dt}-nt{f['nt']}"
    else:
        head = f"f96-{dt}-nt{f['nt']}-gpt{f['gpt']}-{'epi' if f['epi'] else 'plain'}" + (f"-s{f['splits']}-cps{f['cps']}" if f["splits"] > 1 else "")
    if r["refuse"]:
        head = "refuse-" + "+".join(sorted(r["refuse"])) + "-" + head
    return f"{head}{vec}{'-dgrad' if r['dgrad'] else ''}-{r['name']}"


def fwd(name, dt, B, dims, Cin, Cout, form, x="contig", y="contig", res=None, stat=0, sc=None, s2c=0, fs=None, bg=0, defer=0, dgrad=0, refuse=()):
    r = dict(name=name, dt=dt, B=B, dims=tuple(dims), Cin=Cin, Cout=Cout, form=dict(form), lay=dict(x=x, y=y), res=res, stat=stat, sc=sc, s2c=s2c, fs=fs, bg=bg,
             defer=defer, dgrad=dgrad, refuse=frozenset(refuse))
    # whole 16-byte vectors per operand follow from its layout: part of the form (and of the id) without being written out in every row
    auto = dict(vec_x=vec_of(Cin, dt, x), vec_y=vec_of(Cout, dt, y), vec_r=vec_of(Cout, dt, res))
    assert all(r["form"].get(k, v) == v for k, v in auto.items()), (name, r["form"], auto)
    r["form"].update(auto)
    r["id"] = _id(r)
    assert all(r["id"] != o["id"] for o in FWD), r["id"]
    FWD.append(r)


V1, V1E = (5, 9, 17), (6, 10, 18)                    # 12 bricks of 4 x 4 x 16: fewer than 256 workgroups, one 16-channel tile each (nt 1)
V3, V3E, V3B = (14, 15, 60), (14, 16, 60), (8, 16, 64)      # 64 bricks, partial on all three axes (V3B: B = 2): 64 x ceil(192 / 48) = 256 workgroups keep nt 3
V2, V2E = (30, 31, 65), (32, 32, 64)                 # 320 / 256 bricks: nt 2 for 17 .. 32 output channels
RS = dict(res="contig", stat=1)

# ================================================================================================================ 96-byte kernel, unsplit, no epilogue
fwd("48to48", "bf16", 1, V1, 48, 48, F96(1))
fwd("40to48-padded-chunk", "bf16", 1, V1, 40, 48, F96(1))
fwd("32to48", "bf16", 1, V1, 32, 48, F96(1, 4))
fwd("16to48", "bf16", 1, V1, 16, 48, F96(1, 2))
fwd("24to48", "f32", 1, V1, 24, 48, F96(1))
fwd("48to192", "bf16", 1, V3, 48, 192, F96(3))
fwd("48to176-last-tile-32-of-48", "bf16", 1, V3, 48, 176, F96(3))
fwd("48to200-clamped-weight-rows", "bf16", 1, V3, 48, 200, F96(3))
fwd("96to192-two-chunks", "bf16", 1, V3, 96, 192, F96(3, cps=2))
fwd("32to192", "bf16", 1, V3, 32, 192, F96(3, 4))
fwd("64to192-two-chunks", "bf16", 1, V3, 64, 192, F96(3, 4, cps=2))
fwd("16to192", "bf16", 1, V3, 16, 192, F96(3, 2))
fwd("24to192", "f32", 1, V3, 24, 192, F96(3))
fwd("48to24", "bf16", 1, V2, 48, 24, F96(2))
fwd("16to32", "bf16", 1, V2, 16, 32, F96(2, 2))
fwd("32to32", "bf16", 1, V2E, 32, 32, F96(2, 4))
fwd("24to24", "f32", 1, V2, 24, 24, F96(2))
fwd("64to16-320-bricks-two-chunks", "bf16", 1, V2, 64, 16, F96(1, 4, cps=2))
# operands that are not contiguous and aligned: the scalar staging (vec_x 0), scalar stores (vec_y 0); aligned slices keep the vectors
fwd("48to48-x-off8", "bf16", 1, V1, 48, 48, F96(1, vec_x=0), x="off8")
fwd("40to48-x-ldodd-ragged", "bf16", 1, V1, 40, 48, F96(1, vec_x=0), x="ldodd")
fwd("48to48-slices", "bf16", 1, V1, 48, 48, F96(1), x="slice", y="slice")
fwd("24to48-x-off8-y-ldodd", "f32", 1, V1, 24, 48, F96(1, vec_x=0, vec_y=0), x="off8", y="ldodd")
fwd("48to192-x-off8-y-ldodd", "bf16", 1, V3, 48, 192, F96(3, vec_x=0, vec_y=0), x="off8", y="ldodd")

# ================================================================================================================ residual and statistics, unsplit
for _name, _p in (("res", dict(res="contig")), ("stat", dict(stat=1)), ("res-stat", RS)):
    fwd(f"48to48-{_name}", "bf16", 1, V1, 48, 48, F96(1, epi=1), **_p)
    fwd(f"48to192-{_name}", "bf16", 1, V3, 48, 192, F96(3, epi=1), **_p)
    fwd(f"48to24-{_name}", "bf16", 1, V2, 48, 24, F96(2, epi=1), **_p)
fwd("24to48-res-stat", "f32", 1, V1, 24, 48, F96(1, epi=1), **RS)
fwd("24to24-res-stat", "f32", 1, V2, 24, 24, F96(2, epi=1), **RS)
fwd("24to192-res-stat", "f32", 1, V3, 24, 192, F96(3, epi=1), **RS)
fwd("32to48-res-stat", "bf16", 1, V1, 32, 48, F96(1, 4, epi=1), **RS)
fwd("32to32-res-stat", "bf16", 1, V2E, 32, 32, F96(2, 4, epi=1), **RS)
fwd("64to192-res-stat", "bf16", 1, V3, 64, 192, F96(3, 4, epi=1, cps=2), **RS)
fwd("16to48-res-stat", "bf16", 1, V1, 16, 48, F96(1, 2, epi=1), **RS)
fwd("16to32-res-stat", "bf16", 1, V2, 16, 32, F96(2, 2, epi=1), **RS)
fwd("16to192-res-stat", "bf16", 1, V3, 16, 192, F96(3, 2, epi=1), **RS)
fwd("48to192-b2-res-stat", "bf16", 2, V3B, 48, 192, F96(3, epi=1), **RS)      # the statistics' sample index
for _lay in ("slice", "off8", "ldodd"):
    fwd(f"48to48-res-{_lay}-stat", "bf16", 1, V1, 48, 48, F96(1, epi=1, vec_r=int(_lay == "slice")), res=_lay, stat=1)
fwd("48to192-res-off8-stat", "bf16", 1, V3, 48, 192, F96(3, epi=1, vec_r=0), res="off8", stat=1)
fwd("48to48-res-stat-y-off8", "bf16", 1, V1, 48, 48, F96(1, epi=1, vec_y=0), y="off8", **RS)
fwd("48to48-res-stat-y-ldodd", "bf16", 1, V1, 48, 48, F96(1, epi=1, vec_y=0), y="ldodd", **RS)
fwd("48to176-res-stat", "bf16", 1, V3, 48, 176, F96(3, epi=1), **RS)
fwd("48to200-res-stat", "bf16", 1, V3, 48, 200, F96(3, epi=1), **RS)
fwd("48to42-res-stat", "bf16", 1, V1, 48, 42, F96(1, epi=1, vec_y=0, vec_r=0), **RS)      # contiguous rows of 42 channels: no whole vectors
fwd("24to42-res-stat", "f32", 1, V1, 24, 42, F96(1, epi=1, vec_y=0, vec_r=0), **RS)

# ================================================================================================================ the 1x1x1 terms and the space-to-channel store
fwd("48to192-sc48", "bf16", 1, V3, 48, 192, F96(3, epi=1), sc=(48, "contig"))
fwd("48to192-sc96", "bf16", 1, V3, 48, 192, F96(3, epi=1), sc=(96, "contig"))
fwd("48to192-sc48-res", "bf16", 1, V3, 48, 192, F96(3, epi=1), sc=(48, "contig"), res="contig")
fwd("48to176-sc48", "bf16", 1, V3, 48, 176, F96(3, epi=1), sc=(48, "contig"))
fwd("48to48-sc48-res", "bf16", 1, V1, 48, 48, F96(1, epi=1), sc=(48, "contig"), res="contig")
# what _Conv3.backward launches: the shortcut term, the residual and the space-to-channel store in one call
fwd("48to192-sc48-s2c48-res", "bf16", 1, V3E, 48, 192, F96(3, epi=1), sc=(48, "contig"), s2c=48, res="contig")
fwd("48to192-sc96-s2c96-res", "bf16", 1, V3E, 48, 192, F96(3, epi=1), sc=(96, "slice"), s2c=96, res="slice")
fwd("48to48-s2c16", "bf16", 1, V1E, 48, 48, F96(1, epi=1), s2c=16)
fwd("48to192-s2c96-res", "bf16", 1, V3E, 48, 192, F96(3, epi=1), s2c=96, res="contig")
fwd("24to192-s2c48", "f32", 1, V3E, 24, 192, F96(3, epi=1), s2c=48)
# what _Conv3Shortcut launches: the block's 1x1x1 convolution as a second output, each output with its statistics
fwd("48to192-fs", "bf16", 1, V3, 48, 192, F96(3, epi=1), fs=(0, "contig"))
fwd("48to192-fs-stats", "bf16", 1, V3, 48, 192, F96(3, epi=1), fs=(1, "contig"), stat=1)
fwd("48to192-fs-y-slice", "bf16", 1, V3, 48, 192, F96(3, epi=1), fs=(1, "slice"))
fwd("48to192-fs-y-off8", "bf16", 1, V3, 48, 192, F96(3, epi=1), fs=(0, "off8"))
fwd("48to192-fs-res-stat", "bf16", 1, V3, 48, 192, F96(3, epi=1), fs=(1, "contig"), **RS)
fwd("96to192-fs-stats", "bf16", 1, V3, 96, 192, F96(3, epi=1, cps=2), fs=(1, "contig"), stat=1)
fwd("48to48-fs-stats", "bf16", 1, V1, 48, 48, F96(1, epi=1), fs=(1, "contig"), stat=1)
# background = 1: one workgroup per CU (83 KB of LDS asked for), the same arithmetic
fwd("48to48-background", "bf16", 1, V1, 48, 48, F96(1), bg=1)
fwd("32to48-background", "bf16", 1, V1, 32, 48, F96(1, 4), bg=1)
fwd("16to48-background-res-stat", "bf16", 1, V1, 16, 48, F96(1, 2, epi=1), bg=1, **RS)
fwd("48to192-background-res-stat", "bf16", 1, V3, 48, 192, F96(3, epi=1), bg=1, **RS)

# ================================================================================================================ split launches
V12, VC = (12, 12, 12), (14, 15, 30)
_SPLIT = [("192to96", "bf16", V12, 192, 96, F96(1, splits=4)),
          ("128to128", "bf16", V12, 128, 128, F96(1, 4, splits=4)),
          ("130to64-padded-chunk", "bf16", V1, 130, 64, F96(1, splits=3)),
          ("56to48-padded-chunk", "bf16", V1, 56, 48, F96(1, splits=2)),
          ("50to48-padded-chunk", "f32", V1, 50, 48, F96(1, splits=3)),
          ("240to42", "bf16", (5, 7, 18), 240, 42, F96(1, splits=5, vec_y=0)),
          ("120to42", "f32", (5, 7, 18), 120, 42, F96(1, splits=5, vec_y=0)),
          ("240to96-short-last-split", "bf16", VC, 240, 96, F96(1, splits=3, cps=2)),
          ("120to96-short-last-split", "f32", VC, 120, 96, F96(1, splits=3, cps=2)),
          ("320to96-short-last-split", "bf16", VC, 320, 96, F96(1, 4, splits=3, cps=4))]
for _name, _dt, _dims, _ci, _co, _f in _SPLIT:
    fwd(_name, _dt, 1, _dims, _ci, _co, _f)
    if _name not in ("50to48-padded-chunk", "120to96-short-last-split"):      # (fp32 partners whose residual row would repeat the bf16 row's form; 120 -> 42 keeps its)
        fwd(_name + "-res-stat", _dt, 1, _dims, _ci, _co, _f, **RS)
    fwd(_name + "-deferred", _dt, 1, _dims, _ci, _co, _f, stat=1, defer=1)
fwd("56to48-res-defer-is-not-deferred", "bf16", 1, V1, 56, 48, F96(1, splits=2), res="contig", defer=1)
fwd("56to48-y-slice-res-slice-stat", "bf16", 1, V1, 56, 48, F96(1, splits=2), y="slice", res="slice", stat=1)
fwd("56to48-y-off8-res-off8-stat", "bf16", 1, V1, 56, 48, F96(1, splits=2, vec_y=0, vec_r=0), y="off8", res="off8", stat=1)
fwd("50to48-y-ldodd-res-ldodd-stat", "f32", 1, V1, 50, 48, F96(1, splits=3, vec_y=0, vec_r=0), y="ldodd", res="ldodd", stat=1)
fwd("130to64-x-off8", "bf16", 1, V1, 130, 64, F96(1, splits=3, vec_x=0), x="off8")

# ================================================================================================================ the tiny kernel
_TINY = [("1-voxel", 1, (1, 1, 1), 96, 16, TINY(2, 1, 2, 1)),         # three of the four waves leave early
         ("32-voxels", 1, (2, 2, 8), 96, 20, TINY(2, 1, 2, 2)),
         ("30-voxels-b2", 2, (2, 3, 5), 96, 48, TINY(2, 1, 2, 3)),
         ("3x3x3-96to42", 1, (3, 3, 3), 96, 42, TINY(2, 1, 2, 3)),
         ("33-voxels", 1, (1, 3, 11), 96, 48, TINY(4, 4, 2, 3)),
         ("6x6x6-144to40", 1, (6, 6, 6), 144, 40, TINY(4, 4, 3, 3)),
         ("5x7x6-b2-96to96", 2, (5, 7, 6), 96, 96, TINY(4, 4, 2, 1)),
         ("6x6x7-b3-96to50", 3, (6, 6, 7), 96, 50, TINY(4, 4, 2, 1)),
         ("6x6x6-104to48-partial-chunk", 1, (6, 6, 6), 104, 48, TINY(4, 4, 3, 3))]
for _name, _b, _dims, _ci, _co, _f in _TINY:
    fwd(_name, "bf16", _b, _dims, _ci, _co, _f)
for _name, _b, _dims, _ci, _co, _f in _TINY[3:4] + _TINY[6:8]:
    fwd(_name + "-res-stat", "bf16", _b, _dims, _ci, _co, _f, **RS)
fwd("3x3x3-96to42-deferred", "bf16", 1, (3, 3, 3), 96, 42, TINY(2, 1, 2, 3), stat=1, defer=1)
fwd("6x6x7-b3-96to50-deferred", "bf16", 3, (6, 6, 7), 96, 50, TINY(4, 4, 2, 1), stat=1, defer=1)
# ... and what leaves it for the brick kernel with every chunk a split of its own
fwd("not-tiny-6x6x6-100to48-cin-mod-8", "bf16", 1, (6, 6, 6), 100, 48, F96(3, splits=3, vec_x=0))      # (contiguous rows of 100 channels: ldx % 8 != 0)
fwd("not-tiny-4x8x8-lds-bound", "bf16", 1, (4, 8, 8), 96, 48, F96(3, splits=2))
fwd("not-tiny-6x6x6-x-off8", "bf16", 1, (6, 6, 6), 144, 40, F96(3, splits=3, vec_x=0), x="off8")
fwd("not-tiny-3x3x3-background", "bf16", 1, (3, 3, 3), 96, 42, F96(3, splits=2, vec_y=0), bg=1)
fwd("not-tiny-3x3x3-128to48-gpt4", "bf16", 1, (3, 3, 3), 128, 48, F96(3, 4, splits=4))

# ================================================================================================================ the row-major kernel
VR = (5, 9, 11)
fwd("3to16", "f32", 1, VR, 3, 16, RM(1, vec_x=0, vec_y=1))
fwd("8to24", "bf16", 1, VR, 8, 24, RM(2))
fwd("8to40", "f32", 1, VR, 8, 40, RM(3))
fwd("24to100-b2", "bf16", 2, VR, 24, 100, RM(4, vec_y=0))
fwd("20to96", "bf16", 1, VR, 20, 96, RM(6, vec_x=0))
fwd("24to130", "bf16", 1, VR, 24, 130, RM(6, vec_y=0))
fwd("8to24-x-off8-y-ldodd", "bf16", 1, VR, 8, 24, RM(2, vec_x=0, vec_y=0), x="off8", y="ldodd")
fwd("8to40-x-ldodd-y-ldodd", "f32", 1, VR, 8, 40, RM(3, vec_x=0, vec_y=0), x="ldodd", y="ldodd")
fwd("8to24", "bf16", 1, VR, 8, 24, RM(2), res="contig", refuse=["res"])
fwd("8to24", "bf16", 1, VR, 8, 24, RM(2), stat=1, refuse=["stat"])
fwd("24to48", "bf16", 1, (6, 10, 12), 24, 48, RM(3), sc=(48, "contig"), refuse=["sc"])
fwd("24to48", "bf16", 1, (6, 10, 12), 24, 48, RM(3), s2c=16, refuse=["s2c"])
fwd("24to48", "bf16", 1, (6, 10, 12), 24, 48, RM(3), fs=(0, "contig"), refuse=["fs"])

# ================================================================================================================ refusals of the 96-byte kernel
fwd("fp32", "f32", 1, V1, 24, 48, F96(1), sc=(48, "contig"), refuse=["sc"])
fwd("fp32", "f32", 1, V1, 24, 48, F96(1), fs=(0, "contig"), refuse=["fs"])
fwd("split", "bf16", 1, V1, 96, 48, F96(1, splits=2), sc=(48, "contig"), refuse=["sc"])
fwd("split", "bf16", 1, V1, 96, 48, F96(1, splits=2), fs=(1, "contig"), refuse=["fs"])
fwd("gpt4", "bf16", 1, V1, 32, 48, F96(1, 4), sc=(48, "contig"), refuse=["sc"])
fwd("gpt4", "bf16", 1, V1, 32, 48, F96(1, 4), fs=(0, "contig"), refuse=["fs"])
fwd("sc40", "bf16", 1, V1, 48, 48, F96(1), sc=(40, "contig"), refuse=["sc"])
fwd("sc-x-off8", "bf16", 1, V1, 48, 48, F96(1), sc=(48, "off8"), refuse=["sc"])
fwd("x-off8", "bf16", 1, V1, 48, 48, F96(1, vec_x=0), x="off8", fs=(0, "contig"), refuse=["fs"])
fwd("odd-extent", "bf16", 1, V1, 48, 48, F96(1), s2c=16, refuse=["s2c"])
fwd("s2c-covers-every-channel", "bf16", 1, V1E, 48, 48, F96(1), s2c=48, refuse=["s2c"])
fwd("s2c32-is-no-multiple-of-the-tile", "bf16", 1, V3E, 48, 192, F96(3), s2c=32, refuse=["s2c"])

# ================================================================================================================ data gradient (the mirrored pack on dy)
fwd("layer-192to48", "bf16", 1, V3, 48, 192, F96(3), dgrad=1)
fwd("layer-48to40-k-side-padded-on-cout", "bf16", 1, V1, 40, 48, F96(1), dgrad=1)
fwd("layer-48to24", "f32", 1, V1, 24, 48, F96(1), dgrad=1)
fwd("layer-24to48-res", "bf16", 1, V2, 48, 24, F96(2, epi=1), dgrad=1, res="contig")
fwd("layer-64to130", "bf16", 1, V1, 130, 64, F96(1, splits=3), dgrad=1)
fwd("layer-42to240", "bf16", 1, (5, 7, 18), 240, 42, F96(1, splits=5, vec_y=0), dgrad=1)
fwd("layer-96to240", "bf16", 1, VC, 240, 96, F96(1, splits=3, cps=2), dgrad=1)
fwd("layer-42to96", "bf16", 1, (3, 3, 3), 96, 42, TINY(2, 1, 2, 3), dgrad=1)
fwd("layer-40to144", "bf16", 1, (6, 6, 6), 144, 40, TINY(4, 4, 3, 3), dgrad=1)
fwd("layer-24to8", "bf16", 1, VR, 8, 24, RM(2), dgrad=1)

assert len(FWD) <= MAX_ROWS, len(FWD)


# ================================================================================================================ params, form, expectations
def op_layout(r, name):
    """(element offset, leading dimension, channels) of an operand of the row"""
    c = {"x": r["Cin"], "y": r["Cout"], "res": r["Cout"], "sc_x": r["sc"][0] if r["sc"] else 0, "fs_y": r["Cout"]}[name]
    lay = {"x": r["lay"]["x"], "y": r["lay"]["y"], "res": r["res"], "sc_x": r["sc"][1] if r["sc"] else None, "fs_y": r["fs"][1] if r["fs"] else None}[name]
    return layout(c, r["dt"], lay) + (c,)


def standins(r):
    """stand-in addresses with the alignment the row's layouts give the real operands"""
    es = ES[r["dt"]]
    a = dict(x=A + op_layout(r, "x")[0] * es, y=A + op_layout(r, "y")[0] * es, wpk=A, ws=A)
    a["res"] = A + op_layout(r, "res")[0] * es if r["res"] else 0
    a["stat"] = A if r["stat"] else 0
    a["sc_x"], a["sc_w"] = (A + op_layout(r, "sc_x")[0] * es, A) if r["sc"] else (0, 0)
    a["s2c"] = A if r["s2c"] else 0
    a["fs_w"], a["fs_y"], a["fs_stat"] = (A, A + op_layout(r, "fs_y")[0] * es, A if r["fs"][0] else 0) if r["fs"] else (0, 0, 0)
    return a


def params(r, L, a):
    B, (D, H, W) = r["B"], r["dims"]
    p = L.Conv3(a["x"], op_layout(r, "x")[1], a["y"], op_layout(r, "y")[1], a["wpk"], B, D, H, W, r["Cin"], r["Cout"], L.BF16 if r["dt"] == "bf16" else L.F32)
    p.workspace = a["ws"]
    if r["res"]:
        p.res, p.ldres = a["res"], op_layout(r, "res")[1]
    p.stat, p.background, p.defer_slabs = a["stat"], r["bg"], r["defer"]
    if r["sc"]:
        p.sc_x, p.ld_sc_x, p.sc_w, p.sc_C = a["sc_x"], op_layout(r, "sc_x")[1], a["sc_w"], r["sc"][0]
    if r["s2c"]:
        p.s2c_out, p.s2c_C = a["s2c"], r["s2c"]
    if r["fs"]:
        p.fs_w, p.fs_y, p.ld_fs_y, p.fs_stat = a["fs_w"], a["fs_y"], op_layout(r, "fs_y")[1], a["fs_stat"]
    return p


def form(L, prm):
    f = L.Conv3FwdForm()
    return L.load().miseg_conv3_fwd_form(C.byref(prm), C.byref(f)), f


def same_arithmetic(f):
    """launches whose forms agree on this tuple add the same products in the same order"""
    return (f.plan.kernel, f.gpt, f.nt, f.plan.splits, f.cps, f.tiny_mt, f.tiny_mg)


def check_form(r, L, rc, f):
    assert rc == 0, (r["id"], rc, L.load().miseg_last_error())
    w, (D, H, W), B, Cin, Cout = r["form"], r["dims"], r["B"], r["Cin"], r["Cout"]
    kernel = {"F96": L.CONV3_FWD96, "TINY": L.CONV3_FWD_TINY, "RM": L.CONV3_GENERIC}[w["kernel"]]
    assert f.plan.kernel == kernel, f"{r['id']}: the form names kernel {f.plan.kernel}, the row is there for {kernel}"
    fast = w["kernel"] != "RM"
    got = dict(nt=f.nt, gpt=f.gpt, epi=f.epi, splits=f.plan.splits, cps=f.cps, vec_x=f.vec_x, vec_y=f.vec_y, vec_r=f.vec_r, tiny=(f.tiny_mt, f.tiny_mg))
    want = dict(tiny=(0, 0))
    want.update({k: v for k, v in w.items() if k != "kernel"})
    assert got == want, f"{r['id']}: the form says {got} ({f.nchunks} chunks, {f.nbricks} bricks), the row is there for {want}"
    # the pieces: served unless the row says refused; the row-major kernel serves none
    refused = r["refuse"]
    deferred = int(bool(r["defer"]) and f.plan.splits > 1 and not r["res"])
    served = dict(res=int(bool(r["res"]) and fast), stat=int(bool(r["stat"]) and fast and not deferred), sc=int(bool(r["sc"]) and "sc" not in refused),
                  s2c=int(bool(r["s2c"]) and "s2c" not in refused), fs=int(bool(r["fs"]) and "fs" not in refused), defer_slabs=deferred)
    assert {k: getattr(f.plan, k) for k in served} == served, (r["id"], {k: getattr(f.plan, k) for k in served}, served)
    assert refused <= {k for k in PIECES if r[k] and not served[k]}, r["id"]
    vox = B * D * H * W
    assert f.plan.workspace_bytes == (f.plan.splits * vox * Cout * 4 if f.plan.splits > 1 else 0), r["id"]
    assert f.second_launch == int(f.plan.splits > 1 and not deferred), r["id"]
    assert f.vec_fs_y == vec_of(Cout, r["dt"], r["fs"][1] if r["fs"] else None), r["id"]
    if w["kernel"] == "RM":
        cb = cdiv(Cin, nvec(r["dt"])) * 16
        assert (f.chunk_bytes, f.nbricks, f.ny, f.wd) == (cb, B * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 8), 0, 0) and cb <= 48, r["id"]
        assert (f.grid_x, f.grid_y, f.grid_z, f.lds_bytes) == (f.nbricks, cdiv(Cout, 16 * f.nt), 1, 6 * 10 * 10 * (cb + 16)), r["id"]
        return
    assert f.nbricks == B * cdiv(D, 4) * cdiv(H, 4) * cdiv(W, 16) and f.chunk_bytes == 0, r["id"]
    assert f.cps * (f.plan.splits - 1) < f.nchunks <= f.cps * f.plan.splits and f.nchunks == cdiv(cdiv(Cin, nvec(r["dt"])), f.gpt), r["id"]
    if w["kernel"] == "TINY":
        cop16 = cdiv(Cout, 16)
        assert (f.grid_x, f.grid_y, f.grid_z) == (cdiv(cop16, 4) if f.tiny_mg == 1 else cop16, f.nchunks, B) and f.plan.splits == f.nchunks, r["id"]
        assert f.lds_bytes == (D + 2) * (H + 2) * (W + 2) * 112 <= 64 * 1024 and (f.ny, f.wd) == (0, 0), r["id"]
        assert (D * H * W <= 32) == (f.tiny_mg == 1) and D * H * W <= f.tiny_mt * f.tiny_mg * 16, r["id"]
        return
    lds = f.gpt * 656 * 16 + 2 * 12 * 16 * f.nt * 16
    assert f.lds_bytes == (max(lds, 83 * 1024) if r["bg"] else lds), r["id"]
    assert (f.ny, f.wd) == (cdiv(Cout, 16 * f.nt), 2 if f.nt == 2 else 3) and (f.grid_x, f.grid_y, f.grid_z) == (f.nbricks * f.ny, 1, f.plan.splits), r["id"]
