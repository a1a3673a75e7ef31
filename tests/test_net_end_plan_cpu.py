"""The host-only plans of the network-end launchers (miseg_conv3_thin_fwd_plan, miseg_conv3_thin_wgrad_plan, miseg_patch_embed_fwd_plan,
miseg_patch_embed_bwd_plan, miseg_head_fwd_plan, miseg_head_bwd_plan; csrc/net_end.hip): the launchers dispatch on them, so the kernel a
shape reaches is pinned here without a card.  The table is tests/net_end_cases.py - the rows tests/test_hip_net_end_forms.py launches - run
with stand-in addresses (aligned 1 << 12, or 8 bytes into a 16-byte unit): every row asserts the kernel, the partial-sum flag, the passes and,
where the row is there for a wrapping loop, items > workgroups x items per trip.  Every kernel value of every plan appears in a row.
The 64-bit item forms need 2^29 to 2^31 items: they are pinned here on the plan alone and are NOT launched by any test.  CPU only."""
import ctypes as C

import pytest

import net_end_cases as NE


def _L():
    from mi_seg_amd.hip import lib
    return lib


@pytest.mark.parametrize("row", NE.ROWS, ids=lambda r: r["id"])
def test_the_plan_names_the_form_each_row_is_there_for(row):
    L = _L()
    rc, pl = NE.plan(row, L, NE.params(row, L, NE.standins(row)))
    NE.check_plan(row, L, rc, pl)


def test_every_kernel_of_every_plan_is_reached_by_a_row():
    L = _L()
    seen = {fn: set() for fn in NE.PLAN_FN.values()}
    for row in NE.ROWS:
        rc, pl = NE.plan(row, L, NE.params(row, L, NE.standins(row)))
        assert rc == 0
        seen[NE.PLAN_FN[row["op"]]] |= {e.kernel for _, e, _ in NE.launches(row, pl)}
    assert set(seen) == set(L.NE_KERNELS)
    for fn, kernels in L.NE_KERNELS.items():
        assert seen[fn] == set(kernels), f"{fn}: kernels {sorted(set(kernels) - seen[fn])} are reached by no row of the table"
    everything = {v for k, v in vars(L).items() if k.startswith("NE_") and isinstance(v, int)}
    assert everything == set().union(*L.NE_KERNELS.values()) and everything == set(range(18))
    # both sides of every flag the plans report, and a wrapping loop per kernel that has a loop under a workgroup cap
    flags = set()
    wrapped = set()
    for row in NE.ROWS:
        _, pl = NE.plan(row, L, NE.params(row, L, NE.standins(row)))
        for _, e, _ in NE.launches(row, pl):
            flags.add((e.kernel, "partial", e.partial))
            flags.add((e.kernel, "passes", e.passes))
            if NE.wraps(e):
                wrapped.add(e.kernel)
    for k in (L.NE_STEM_WGRAD_MFMA, L.NE_PATCH_BWD_TEAM):
        assert (k, "partial", 0) in flags and (k, "partial", 1) in flags
    assert (L.NE_HEAD_DW_TEAM, "passes", 1) in flags and (L.NE_HEAD_DW_TEAM, "passes", 2) in flags
    assert wrapped == {L.NE_STEM_FWD_GENERIC, L.NE_STEM_FWD_BRICK, L.NE_STEM_FWD_MFMA, L.NE_STEM_WGRAD_BRICK, L.NE_STEM_WGRAD_MFMA, L.NE_PATCH_FWD,
                       L.NE_HEAD_FWD_SCALAR, L.NE_HEAD_FWD_TILE, L.NE_HEAD_DX_SCALAR, L.NE_HEAD_DX_TEAM, L.NE_HEAD_DX_TILE, L.NE_HEAD_DW_MFMA}


def test_workgroup_counts_and_the_partial_sum_threshold():
    """the figures the table's shapes were chosen by: caps 2048 / 4096 / 512 bricks, 1152 / 512 tiles, 8192 workgroups; 16 workgroups for partial sums"""
    L = _L()
    by_id = {r["id"]: r for r in NE.ROWS}

    def launch(rid, which=0):
        r = by_id[rid]
        rc, pl = NE.plan(r, L, NE.params(r, L, NE.standins(r)))
        assert rc == 0
        e = NE.launches(r, pl)[which][1]
        return e.workgroups, e.per_workgroup, e.items

    assert launch("stem_fwd-mfma-wrap-2197-bricks-bf16") == (2048, 1, 2197)
    assert launch("stem_fwd-brick-wrap-4624-bricks-f32") == (4096, 1, 4624)
    assert launch("stem_fwd-generic-wrap-2113536-voxels-f32") == (8192, 256, 2113536)
    assert launch("stem_wgrad-mfma-12wg-atomics-bf16") == (12, 1, 12)
    assert launch("stem_wgrad-mfma-18wg-partial-bf16") == (18, 1, 18)
    assert launch("stem_wgrad-mfma-b2-ragged-bf16") == (16, 1, 16)
    assert launch("stem_wgrad-mfma-wrap-648-bricks-bf16") == (512, 1, 648)
    assert launch("stem_wgrad-brick-wrap-648-bricks-f32") == (512, 1, 648)
    assert launch("patch_fwd-wrap-2116800-items-bf16") == (8192, 256, 2116800)
    assert launch("patch_bwd-team-cout24-15wg-atomics-f32") == (15, 168, 2520) == launch("patch_bwd-team-cout48-15wg-atomics-bf16")
    assert launch("patch_bwd-team-cout24-16wg-partial-f32") == (16, 168, 2548) == launch("patch_bwd-team-cout48-16wg-partial-bf16")
    assert launch("patch_bwd-generic-cin4-3blocks-f32") == (3, 1024, 2520)
    assert launch("head_fwd-tile-wrap-1175-tiles-bf16") == (588, 1, 1175)      # two rounds, balanced: ceil(1175 / 2)
    assert launch("head_fwd-scalar-wrap-2113536-voxels-bf16") == (8192, 256, 2113536) == launch("head_bwd-scalar-wrap-2113536-voxels-f32", 0)
    assert launch("head_bwd-dxtile-dwmfma-wrap-1168-tiles-bf16", 0) == (584, 1, 1168)
    assert launch("head_bwd-dxtile-dwmfma-wrap-1168-tiles-bf16", 1) == (390, 1, 1168)      # three rounds under the cap of 512
    assert launch("head_bwd-dxteam-wrap-2107392-items-f32", 0) == (8192, 256, 2107392)
    assert launch("head_bwd-dwteam-3-rows-bf16", 1) == (1, 168, 3)
    assert launch("head_bwd-scalar-16-blocks-of-64-f32", 1) == (2, 2048, 2976)


def test_the_64_bit_item_forms_are_chosen_by_size_alone():
    """Not launched anywhere: the 64-bit instantiations of patch_embed_fwd_kernel and head_bwd_dx_team_kernel need 2^31 - 2^21 work items
    (or an input of 2^31 elements), resp. 2^29 items - tens of GB of operands.  The plans are asked with large shapes and stand-in pointers."""
    L = _L()
    A = NE.A
    lib = L.load()

    def patch(B, Cin, D, H, W, Cout):
        pl = L.NetEndLaunch()
        assert lib.miseg_patch_embed_fwd_plan(C.byref(L.PatchEmbed(A, A, Cout, A, A, B, Cin, D, H, W, Cout, L.BF16)), C.byref(pl)) == 0
        return pl

    assert patch(1, 1, 1024, 1024, 1024, 48).idx32 == 1      # 2^27 coarse voxels x 6 groups, 2^30 inputs
    assert patch(2, 1, 1024, 1024, 1024, 48).idx32 == 0      # 2^31 input elements
    assert patch(1, 1, 1024, 1024, 1024, 128).idx32 == 0     # 2^31 items
    near = patch(1, 1, 1024, 2046, 512, 127)
    assert near.items == (1 << 31) - (1 << 21) and near.idx32 == 0      # fits 31 bits, but the last trip's index may overshoot by a grid of 2^21
    assert patch(1, 1, 1024, 2044, 512, 127).idx32 == 1

    def dx(B, S, Cin, dt):
        pl = L.HeadBwdPlan()
        assert lib.miseg_head_bwd_plan(C.byref(L.HeadBwd(A, Cin, A, A, Cin, A, A, A, B, S, Cin, 9, dt)), C.byref(pl)) == 0
        assert pl.dx.kernel == L.NE_HEAD_DX_TEAM and pl.dx.workgroups == 8192
        return pl.dx

    assert dx(1, (1 << 29) // 12 + 1, 48, L.F32).idx32 == 0 and dx(1, (1 << 29) // 12, 48, L.F32).idx32 == 1
    assert dx(4, 1 << 24, 64, L.BF16).idx32 == 0 and dx(4, (1 << 24) - 1, 64, L.BF16).idx32 == 1


def test_each_predicate_alone_leaves_the_fast_form():
    """one clause of a launcher's predicate broken at a time, on otherwise fast shapes"""
    L = _L()
    A, lib = NE.A, L.load()

    def k(fn, prm, which=None):
        pl = L.HeadBwdPlan() if fn == "miseg_head_bwd_plan" else L.NetEndLaunch()
        assert getattr(lib, fn)(C.byref(prm), C.byref(pl)) == 0
        return getattr(pl, which).kernel if which else pl.kernel

    def stem(dt=L.BF16, y=A, ld=48, Cin=1, Cout=48):
        return k("miseg_conv3_thin_fwd_plan", L.Conv3Thin(A, y, ld, A, 1, Cin, 8, 8, 16, Cout, dt))

    assert stem() == L.NE_STEM_FWD_MFMA and stem(y=A + 8, ld=52) == L.NE_STEM_FWD_MFMA
    assert stem(y=A + 4) == stem(ld=50) == stem(Cin=2) == L.NE_STEM_FWD_GENERIC
    assert stem(dt=L.F32) == stem(Cout=40) == stem(Cout=64) == L.NE_STEM_FWD_BRICK
    assert stem(Cout=72) == stem(Cout=20) == stem(Cout=24, ld=28) == stem(Cout=24, y=A + 8) == L.NE_STEM_FWD_GENERIC

    def wgrad(dt=L.BF16, dy=A, ld=48, Cin=1, Cout=48):
        return k("miseg_conv3_thin_wgrad_plan", L.Conv3ThinWgrad(A, dy, ld, A, 1, Cin, 8, 8, 16, Cout, dt, A))

    assert wgrad() == L.NE_STEM_WGRAD_MFMA and wgrad(dt=L.F32) == wgrad(Cout=56) == wgrad(Cout=8) == L.NE_STEM_WGRAD_BRICK
    assert wgrad(dy=A + 8) == wgrad(ld=52) == wgrad(Cin=2) == wgrad(Cout=64) == wgrad(Cout=20) == wgrad(dt=L.F32, Cout=24, ld=26) == L.NE_STEM_WGRAD_GENERIC

    def pbwd(dt=L.BF16, dy=A, ld=48, Cout=48):
        return k("miseg_patch_embed_bwd_plan", L.PatchEmbedBwd(A, dy, ld, A, A, 1, 1, 8, 8, 8, Cout, dt, A))

    assert pbwd() == pbwd(dt=L.F32) == pbwd(Cout=8) == L.NE_PATCH_BWD_TEAM
    assert pbwd(dy=A + 8) == pbwd(ld=52) == pbwd(Cout=20) == pbwd(dt=L.F32, Cout=22, ld=24) == L.NE_PATCH_BWD_GENERIC

    def hfwd(dt=L.BF16, x=A, ld=48, Cin=48):
        return k("miseg_head_fwd_plan", L.Head(x, ld, A, A, A, 1, 512, Cin, 6, dt))

    assert hfwd() == hfwd(dt=L.F32) == hfwd(ld=56) == L.NE_HEAD_FWD_TILE
    assert hfwd(x=A + 8) == hfwd(ld=52) == hfwd(Cin=52) == hfwd(dt=L.F32, Cin=50, ld=52) == L.NE_HEAD_FWD_SCALAR

    def hbwd(which, dt=L.BF16, x=A, ldx=48, dx=A, lddx=48, Cin=48, Cout=6, S=512, dy=A):
        return k("miseg_head_bwd_plan", L.HeadBwd(x, ldx, dy, dx, lddx, A, A, A, 1, S, Cin, Cout, dt), which)

    assert hbwd("dx") == L.NE_HEAD_DX_TILE and hbwd("dx", Cin=256, Cout=2) == L.NE_HEAD_DX_TILE
    assert hbwd("dx", dt=L.F32) == hbwd("dx", Cout=9) == hbwd("dx", S=500) == hbwd("dx", Cin=264, Cout=2) == L.NE_HEAD_DX_TEAM
    assert hbwd("dx", dx=A + 8) == hbwd("dx", lddx=52) == hbwd("dx", Cin=52) == L.NE_HEAD_DX_SCALAR and hbwd("dx", dx=0) == L.NE_NONE
    assert hbwd("dw") == hbwd("dw", Cout=16, dx=0) == L.NE_HEAD_DW_MFMA
    assert hbwd("dw", dt=L.F32) == hbwd("dw", S=500) == hbwd("dw", Cin=96) == hbwd("dw", dy=A + 8) == L.NE_HEAD_DW_TEAM
    assert hbwd("dw", x=A + 8) == hbwd("dw", ldx=52) == hbwd("dw", Cin=52) == L.NE_HEAD_DW_GENERIC
    assert hbwd("dw", dt=L.F32, Cin=260, Cout=2) == L.NE_HEAD_DW_GENERIC      # 65 vectors: more than the team's 64 columns


def test_a_refused_problem_gets_the_calls_error_code_from_the_plan():
    """no device is touched: the calls below are refused on the host, before any launch (stream NULL)"""
    L = _L()
    A, lib = NE.A, L.load()
    BADARG, UNSUPPORTED = -1, -2
    cases = [
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, A, 24, A, A, 1, 1, 8, 9, 8, 24, L.BF16), BADARG),            # an odd grid side
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, A, 24, A, A, 1, 1, 7, 8, 8, 24, L.F32), BADARG),
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, A, 24, A, A, 1, 1, 8, 8, 6 + 1, 24, L.F32), BADARG),
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, A, 376, A, A, 1, 4, 8, 8, 8, 376, L.BF16), UNSUPPORTED),      # Cin * 8 * Cout = 12032 > 12000
        ("miseg_patch_embed_fwd", L.PatchEmbed(0, A, 24, A, A, 1, 1, 8, 8, 8, 24, L.BF16), BADARG),
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, 0, 24, A, A, 1, 1, 8, 8, 8, 24, L.BF16), BADARG),
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, A, 24, 0, A, 1, 1, 8, 8, 8, 24, L.BF16), BADARG),
        ("miseg_patch_embed_fwd", L.PatchEmbed(A, A, 24, A, A, 1, 1, 8, 8, 8, 24, 7), BADARG),                  # unknown dtype
        ("miseg_patch_embed_bwd", L.PatchEmbedBwd(A, A, 64, A, A, 1, 4, 8, 8, 8, 64, L.BF16, A), UNSUPPORTED),  # Cout * (8 Cin + 1) = 2112 > 2048
        ("miseg_patch_embed_bwd", L.PatchEmbedBwd(A, A, 24, 0, A, 1, 1, 8, 8, 8, 24, L.BF16, A), BADARG),
        ("miseg_patch_embed_bwd", L.PatchEmbedBwd(A, 0, 24, A, A, 1, 1, 8, 8, 8, 24, L.BF16, A), BADARG),
        ("miseg_conv3_thin_fwd", L.Conv3Thin(A, A, 24, A, 1, 5, 8, 8, 8, 24, L.BF16), UNSUPPORTED),             # Cin 5
        ("miseg_conv3_thin_fwd", L.Conv3Thin(A, A, 24, A, 1, 0, 8, 8, 8, 24, L.BF16), UNSUPPORTED),
        ("miseg_conv3_thin_fwd", L.Conv3Thin(A, A, 140, A, 1, 4, 8, 8, 8, 140, L.F32), UNSUPPORTED),            # Cin * 27 * Cout = 15120 > 15000
        ("miseg_conv3_thin_fwd", L.Conv3Thin(A, 0, 24, A, 1, 1, 8, 8, 8, 24, L.BF16), BADARG),
        ("miseg_conv3_thin_wgrad", L.Conv3ThinWgrad(A, A, 24, A, 1, 5, 8, 8, 8, 24, L.BF16, A), UNSUPPORTED),
        ("miseg_conv3_thin_wgrad", L.Conv3ThinWgrad(A, A, 72, A, 1, 1, 8, 8, 8, 72, L.BF16, A), UNSUPPORTED),   # Cout 72 > 64
        ("miseg_conv3_thin_wgrad", L.Conv3ThinWgrad(A, A, 24, 0, 1, 1, 8, 8, 8, 24, L.BF16, A), BADARG),
        ("miseg_head_fwd", L.Head(A, 48, A, A, A, 1, 512, 48, 17, L.BF16), UNSUPPORTED),                        # Cout 17
        ("miseg_head_fwd", L.Head(A, 520, A, A, A, 1, 512, 520, 16, L.BF16), UNSUPPORTED),                      # Cin * Cout = 8320 > 8192
        ("miseg_head_fwd", L.Head(A, 48, 0, A, A, 1, 512, 48, 6, L.BF16), BADARG),
        ("miseg_head_bwd", L.HeadBwd(A, 48, A, A, 48, A, A, A, 1, 512, 48, 17, L.BF16), UNSUPPORTED),
        ("miseg_head_bwd", L.HeadBwd(A, 64, A, A, 64, A, A, A, 1, 512, 64, 16, L.BF16), UNSUPPORTED),            # Cout * (Cin + 1) = 1040 > 1024
        ("miseg_head_bwd", L.HeadBwd(A, 48, 0, A, 48, A, A, A, 1, 512, 48, 6, L.BF16), BADARG),
        ("miseg_head_bwd", L.HeadBwd(A, 48, A, A, 48, 0, A, A, 1, 512, 48, 6, L.BF16), BADARG),
        ("miseg_head_bwd", L.HeadBwd(A, 48, A, A, 48, A, A, A, 1, 512, 48, 6, 3), BADARG),
    ]
    for fn, prm, code in cases:
        pl = L.HeadBwdPlan() if fn == "miseg_head_bwd" else L.NetEndLaunch()
        assert getattr(lib, fn + "_plan")(C.byref(prm), C.byref(pl)) == code, (fn, lib.miseg_last_error())
        assert getattr(lib, fn)(C.byref(prm), None) == code, (fn, lib.miseg_last_error())
        assert getattr(lib, fn + "_plan")(C.byref(prm), None) == BADARG
        assert getattr(lib, fn + "_plan")(None, C.byref(pl)) == BADARG == getattr(lib, fn)(None, None)
