"""The launch forms of the 3x3x3 forward / data-gradient kernels, host only (miseg_conv3_fwd_form: the struct conv3_fwd_launch of csrc/conv3d.hip
dispatches on - the launcher holds no integer arithmetic of its own): every row of tests/conv3_fwd_cases.py answers the form its id carries, the
form agrees with the public plan on the rows and on the bench shapes of tests/test_conv3_plan.py, every instantiation the launcher can pick is
reached by some row, and a sweep over channel counts, volumes, batches, pieces and base alignments runs the only host arithmetic the launch has:
no grid extent, LDS size or divisor is ever 0, the tiny kernel never gets more than 252 voxels (its LDS bound), the row-major kernel never a
row of more than 48 bytes (so its chunk is the row), the space-to-channel store is never served with two tiles per workgroup, and the workspace
is exactly the slabs of the plan's splits.  CPU only: the form call touches no device; tests/test_hip_conv3_fwd_forms.py launches the same rows
on the card.  Wall time: 1.4 s for the 166 cases (the sweep makes 43 264 form calls)."""
import ctypes as C

import pytest

import conv3_fwd_cases as K
from test_conv3_plan import FWD_ROWS

A = K.A


def _L():
    from mi_seg_amd.hip import lib
    return lib


def _form(r):
    L = _L()
    return K.form(L, K.params(r, L, K.standins(r)))


def _public(pl):
    return (pl.kernel, pl.splits, pl.workspace_bytes, pl.res, pl.stat, pl.sc, pl.s2c, pl.fs, pl.defer_slabs)


def _pieces(r):
    return tuple(k for k in K.PIECES if r[k] and k not in r["refuse"])


@pytest.mark.parametrize("r", K.FWD, ids=lambda r: r["id"])
def test_row_takes_the_form_its_id_names(r):
    L = _L()
    rc, f = _form(r)
    K.check_form(r, L, rc, f)
    pl = L.Conv3Plan()
    assert L.load().miseg_conv3_fwd_plan(C.byref(K.params(r, L, K.standins(r))), C.byref(pl)) == 0
    assert _public(pl) == _public(f.plan), r["id"]


def test_the_table_stays_small():
    assert len(K.FWD) <= K.MAX_ROWS and max(r["B"] * r["dims"][0] * r["dims"][1] * r["dims"][2] for r in K.FWD) <= 66000


def test_every_form_the_launcher_can_pick_is_reached():
    L = _L()
    inst, tiny, rm, vec0, split, combos, bg, second = set(), set(), set(), set(), set(), set(), set(), set()
    for r in K.FWD:
        _, f = _form(r)
        if r["refuse"]:
            continue
        if f.plan.kernel == L.CONV3_FWD96:
            inst.add((r["dt"], f.nt, f.epi, f.gpt))
            vec0 |= {(k, int(f.plan.splits > 1)) for k in ("vec_x", "vec_y", "vec_r") if not getattr(f, k) and (k != "vec_r" or r["res"])}
            if f.plan.splits > 1:
                split.add((r["dt"], f.gpt, int(f.cps > 1), int(f.nchunks % f.cps != 0), f.plan.defer_slabs, int(bool(r["res"]))))
                second |= {(f.second_launch, f.vec_y, f.vec_r if r["res"] else None)}
            else:
                combos.add((f.nt,) + _pieces(r))
            if r["bg"]:
                bg.add((f.gpt, f.nt, int(f.plan.splits > 1)))
        elif f.plan.kernel == L.CONV3_FWD_TINY:
            tiny.add((f.tiny_mt, f.tiny_mg, f.plan.defer_slabs, int(bool(r["res"])), int(r["Cout"] % 4 != 0)))
        else:
            rm.add((r["dt"], f.nt, f.vec_x))
    # every conv3_fwd96_kernel<T, NT, WD, EPI, GPT> the launcher can name: fp32 keeps 96-byte chunks (gpt 6); WD follows NT
    assert inst == {("bf16", nt, e, g) for nt in (1, 2, 3) for e in (0, 1) for g in (6, 4, 2)} | {("f32", nt, e, 6) for nt in (1, 2, 3) for e in (0, 1)}, sorted(inst)
    assert {(mt, mg) for mt, mg, _, _, _ in tiny} == {(2, 1), (4, 4)}
    for k in ((2, 1), (4, 4)):      # each tiny kernel: slabs of Cout % 4 != 0, the second launch with a residual, and deferred
        assert {(d, rs, c4) for mt, mg, d, rs, c4 in tiny if (mt, mg) == k} >= {(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1)}, (k, sorted(tiny))
    assert {nt for _, nt, _ in rm} == {1, 2, 3, 4, 6} and {(dt, vx) for dt, _, vx in rm} == {("bf16", 0), ("bf16", 1), ("f32", 0), ("f32", 1)}, sorted(rm)
    assert vec0 >= {("vec_x", 0), ("vec_y", 0), ("vec_r", 0), ("vec_x", 1), ("vec_y", 1), ("vec_r", 1)}, sorted(vec0)
    # split launches: one and several chunks per split with a shorter last split, both dtypes, 64-byte chunks, plain / residual / deferred
    assert {(dt, g, c, short) for dt, g, c, short, _, _ in split} >= {("bf16", 6, 0, 0), ("bf16", 4, 0, 0), ("f32", 6, 0, 0), ("bf16", 6, 1, 1), ("f32", 6, 1, 1),
                                                                     ("bf16", 4, 1, 1)}, sorted(split)
    forms = {("bf16", 6, 0), ("bf16", 4, 0), ("f32", 6, 0), ("bf16", 6, 1), ("f32", 6, 1), ("bf16", 4, 1)}      # (dtype, gpt, several chunks per split)
    for d, rs in ((0, 0), (1, 0)):      # every split form plain and deferred; with the residual every one but fp32 cps > 1
        assert {(dt, g, c) for dt, g, c, _, d_, rs_ in split if (d_, rs_) == (d, rs)} >= forms, (d, rs, sorted(split))
    assert {(dt, g, c) for dt, g, c, _, d_, rs_ in split if (d_, rs_) == (0, 1)} >= forms - {("f32", 6, 1)}, sorted(split)
    deferred = [r for r in K.FWD if r["defer"] and not r["res"] and r["form"]["kernel"] == "F96"]
    assert {(r["dt"], r["Cout"] % 4 != 0) for r in deferred} >= {("bf16", True), ("f32", True), ("bf16", False), ("f32", False)}
    assert second >= {(1, 1, None), (1, 1, 1), (1, 0, 0), (0, 1, None)}, second
    # every piece alone, and the combinations the model launches (_Conv3.backward: sc + s2c + res; _Conv3Shortcut: fs with both statistics)
    want = {(nt,) + p for nt in (1, 2, 3) for p in ((), ("res",), ("stat",), ("res", "stat"))}
    want |= {(3, "sc"), (3, "res", "sc"), (1, "res", "sc"), (3, "res", "sc", "s2c"), (1, "s2c"), (3, "s2c"), (3, "res", "s2c"), (3, "fs"), (3, "stat", "fs"),
             (1, "stat", "fs"), (3, "res", "stat", "fs")}
    assert combos >= want, sorted(want - combos)
    assert {g for g, _, s in bg if not s} == {6, 4, 2} and (6, 3, 0) in bg, sorted(bg)


def test_the_form_agrees_with_the_plan_on_the_bench_shapes():
    L = _L()
    lib = L.load()
    for dt, S, Cin, Cout, kernel, splits, _, sc, s2c, fs in FWD_ROWS:
        p = L.Conv3(A, Cin, A, Cout, A, 1, S, S, S, Cin, Cout, dt)
        p.sc_x, p.ld_sc_x, p.sc_w, p.sc_C = A, Cin, A, Cin
        p.s2c_out, p.s2c_C = A, Cout // 2
        p.fs_w, p.fs_y, p.ld_fs_y = A, A, Cout
        f, pl = L.Conv3FwdForm(), L.Conv3Plan()
        assert lib.miseg_conv3_fwd_form(C.byref(p), C.byref(f)) == 0 and lib.miseg_conv3_fwd_plan(C.byref(p), C.byref(pl)) == 0
        assert _public(f.plan) == _public(pl) and (pl.kernel, pl.splits, pl.sc, pl.s2c, pl.fs) == (kernel, splits, sc, s2c, fs)
        assert f.epi == int(splits == 1 and bool(sc or s2c or fs)) and f.nt in (1, 2, 3) and (f.ny > 0) == (kernel == L.CONV3_FWD96)
    # the step's largest launch: the data gradient 48 -> 96 at 96^3 with the shortcut term, the residual and the space-to-channel store
    p = L.Conv3(A, 48, A, 96, A, 1, 96, 96, 96, 48, 96, L.BF16)
    p.res, p.ldres, p.sc_x, p.ld_sc_x, p.sc_w, p.sc_C, p.s2c_out, p.s2c_C = A, 96, A, 48, A, 48, A, 48
    f = L.Conv3FwdForm()
    assert lib.miseg_conv3_fwd_form(C.byref(p), C.byref(f)) == 0
    assert (f.nt, f.wd, f.epi, f.gpt, f.ny, f.nbricks, f.grid_x) == (3, 3, 1, 6, 2, 3456, 6912) and (f.plan.res, f.plan.sc, f.plan.s2c) == (1, 1, 1)


VOLUMES = [(1, 1, 1), (1, 1, 2), (2, 2, 8), (3, 3, 3), (6, 6, 6), (6, 6, 7), (4, 8, 8), (2, 4, 32), (12, 12, 12), (5, 9, 17), (14, 16, 60), (33, 31, 65), (96, 96, 96)]
CHANNELS = sorted(set(range(1, 801, 17)) | {16, 32, 48, 800})      # 17 is coprime with 48: its 48 values hit every residue mod 48; and the narrow-chunk widths


def _sweep_params(L, dt, Cin, Cout, k):
    """the k-th variation of a (dtype, Cin, Cout) cell: volume, batch, pieces and base alignments all move with k"""
    D, H, W = VOLUMES[k % len(VOLUMES)]
    B = (1, 2, 64)[(k // len(VOLUMES)) % 3]
    bits = (k * 2654435761 >> 7) & 0x3FF
    off = lambda b: A + (8 if bits >> b & 1 else 0)      # noqa: E731  (an aligned or an 8-byte base)
    p = L.Conv3(off(0), Cin + (bits >> 1 & 1), off(2), Cout, A, B, D, H, W, Cin, Cout, dt)
    p.workspace = A
    if bits >> 3 & 1:
        p.res, p.ldres = off(4), Cout
    p.stat = A if bits >> 5 & 1 else 0
    p.background, p.defer_slabs = bits >> 6 & 1, int(bits & 0x300 == 0x300)
    if bits >> 7 & 1:
        p.sc_C = (48, 96, 40, 24)[k % 4]
        p.sc_x, p.ld_sc_x, p.sc_w = off(1), p.sc_C, A
        p.s2c_out, p.s2c_C = A, (16, 32, 48, 96, 8)[k % 5]
    if bits >> 8 & 1:
        p.fs_w, p.fs_y, p.ld_fs_y, p.fs_stat = A, off(4), Cout, A
    return p


def test_sweep_the_launch_has_no_empty_grid_and_no_zero_divisor():
    L = _L()
    lib = L.load()
    f = L.Conv3FwdForm()
    seen, served, calls = set(), set(), 0
    for dt in (L.BF16, L.F32):
        for i, Cin in enumerate(CHANNELS):
            for j, Cout in enumerate(CHANNELS):
                for k in range(8):
                    p = _sweep_params(L, dt, Cin, Cout, 5 * i + 11 * j + 41 * k)
                    assert lib.miseg_conv3_fwd_form(C.byref(p), C.byref(f)) == 0
                    calls += 1
                    what = (dt, p.B, p.D, p.H, p.W, Cin, Cout)
                    nvox, kpc = p.D * p.H * p.W, 8 if dt == L.BF16 else 4
                    assert min(f.grid_x, f.grid_y, f.grid_z, f.lds_bytes) >= 1 and max(f.grid_y, f.grid_z) <= 65535 and f.lds_bytes <= 160 * 1024, what
                    assert f.plan.splits >= 1 and f.plan.workspace_bytes == (f.plan.splits * p.B * nvox * Cout * 4 if f.plan.splits > 1 else 0), what
                    assert f.second_launch == int(f.plan.splits > 1 and not f.plan.defer_slabs), what
                    if f.plan.kernel == L.CONV3_GENERIC:
                        assert f.nt in (1, 2, 3, 4, 6) and 16 <= f.chunk_bytes <= 48 and f.chunk_bytes == -(-Cin // kpc) * 16, what
                        assert (f.plan.res, f.plan.stat, f.plan.sc, f.plan.s2c, f.plan.fs, f.plan.defer_slabs, f.plan.splits) == (0, 0, 0, 0, 0, 0, 1), what
                        assert f.grid_y == -(-Cout // (16 * f.nt)), what
                    else:
                        assert f.nt in (1, 2, 3) and f.gpt in (2, 4, 6) and f.cps >= 1 and f.nchunks >= 1, what
                        assert f.cps * (f.plan.splits - 1) < f.nchunks <= f.cps * f.plan.splits, what
                        if f.plan.kernel == L.CONV3_FWD_TINY:
                            assert nvox <= 252 and nvox <= 16 * f.tiny_mt * f.tiny_mg and f.lds_bytes <= 64 * 1024, what      # 256 voxels never fit the 64 KB
                            assert (f.tiny_mt, f.tiny_mg) in ((2, 1), (4, 4)) and (f.grid_y, f.grid_z) == (f.nchunks, p.B) and not p.background, what
                            assert f.grid_x * (4 if f.tiny_mg == 1 else 1) * 16 >= Cout, what
                        else:
                            assert f.ny == -(-Cout // (16 * f.nt)) and f.grid_x == f.nbricks * f.ny and f.grid_z == f.plan.splits and f.wd in (2, 3), what
                            assert (f.tiny_mt, f.tiny_mg) == (0, 0), what
                        assert not (f.plan.s2c and f.nt == 2), what      # s2c_C % 32 == 0 and s2c_C < Cout <= 32 has no solution
                        assert f.epi == int(f.plan.splits == 1 and f.plan.kernel == L.CONV3_FWD96 and bool(f.plan.res or f.plan.stat or f.plan.sc or f.plan.s2c or f.plan.fs)), what
                    seen.add((f.plan.kernel, f.nt, f.gpt))
                    served |= {k_ for k_ in ("res", "stat", "sc", "s2c", "fs", "defer_slabs") if getattr(f.plan, k_)}
    assert calls == 2 * len(CHANNELS) ** 2 * 8
    assert {k for k, _, _ in seen} == {L.CONV3_GENERIC, L.CONV3_FWD96, L.CONV3_FWD_TINY} and served == {"res", "stat", "sc", "s2c", "fs", "defer_slabs"}, (seen, served)
    assert {(nt, g) for k, nt, g in seen if k == L.CONV3_FWD96} == {(nt, g) for nt in (1, 2, 3) for g in (2, 4, 6)}


def test_the_row_major_kernel_sees_rows_of_at_most_48_bytes():
    """every channel count: rows of 64 bytes and more are on the 96-byte-chunk path (padded where no chunk width divides them), so the row-major
    launcher stages the whole row as one chunk"""
    L = _L()
    lib = L.load()
    f = L.Conv3FwdForm()
    rm = {L.BF16: set(), L.F32: set()}
    for dt in rm:
        for Cin in range(1, 1025):
            assert lib.miseg_conv3_fwd_form(C.byref(L.Conv3(A, Cin, A, 16, A, 1, 5, 9, 11, Cin, 16, dt)), C.byref(f)) == 0
            if f.plan.kernel == L.CONV3_GENERIC:
                rm[dt].add(Cin)
                assert f.chunk_bytes <= 48
    assert rm[L.BF16] == set(range(1, 9)) | set(range(17, 25)) and rm[L.F32] == set(range(1, 13))


def test_the_form_call_refuses_bad_params():
    L = _L()
    lib = L.load()
    f = L.Conv3FwdForm()
    ok = L.Conv3(A, 48, A, 48, A, 1, 8, 8, 8, 48, 48, L.BF16)
    assert lib.miseg_conv3_fwd_form(C.byref(ok), C.byref(f)) == 0
    assert lib.miseg_conv3_fwd_form(None, C.byref(f)) != 0 and lib.miseg_conv3_fwd_form(C.byref(ok), None) != 0
    assert lib.miseg_conv3_fwd_form(C.byref(L.Conv3(A, 48, A, 48, A, 1, 8, 8, 8, 48, 48, 7)), C.byref(f)) != 0      # unknown dtype
    assert lib.miseg_conv3_fwd_form(C.byref(L.Conv3(A, 48, A, 48, A, 1, 0, 8, 8, 48, 48, L.BF16)), C.byref(f)) != 0      # empty volume
    assert lib.miseg_conv3_fwd_form(C.byref(L.Conv3(A, 40, A, 48, A, 1, 8, 8, 8, 48, 48, L.BF16)), C.byref(f)) != 0      # ldx < Cin
