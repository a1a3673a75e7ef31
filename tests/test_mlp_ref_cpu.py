"""The fused MLP's launch-form table (tests/mlp_cases.py) on the host: its float64 reference against torch's own GELU and autograd, the range
conditions of the exact-integer case, the grid arithmetic every row's id claims, and that the rows name all 12 instantiations of csrc/mlp.hip.
tests/test_hip_mlp_forms.py launches the rows on the card."""
import torch
import torch.nn.functional as F

import mlp_cases as M


def test_reference_agrees_with_torch_gelu_and_autograd_in_float64():
    g = torch.Generator().manual_seed(3)
    n, C, H = 37, 48, 192
    x, res, dy = (torch.randn(n, C, generator=g).to(torch.bfloat16) for _ in range(3))
    w1, w2 = (torch.randn(H, C, generator=g) / C ** 0.5).to(torch.bfloat16), (torch.randn(C, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    b1, b2 = torch.randn(H, generator=g) * 3, torch.randn(C, generator=g)      # (b1 wide: z out to about +-10)
    r = M.reference(x, w1, b1, w2, b2, res, dy)
    z = (x.double() @ w1.double().t() + b1.double()).requires_grad_(True)
    h = F.gelu(z)
    assert float(z.detach().abs().max()) > 8
    assert torch.allclose(r["h"], h.detach(), rtol=1e-13, atol=1e-15)
    y = h.detach().to(torch.bfloat16).double() @ w2.double().t() + b2.double() + res.double()
    assert torch.allclose(r["y"], y, rtol=1e-13, atol=1e-13)
    (dz,) = torch.autograd.grad(h, z, dy.double() @ w2.double())
    assert torch.allclose(r["dz"], dz, rtol=1e-12, atol=1e-15)
    # without the optional terms
    r0 = M.reference(x, w1, None, w2, None, None)
    assert torch.allclose(r0["y"], F.gelu(x.double() @ w1.double().t()).to(torch.bfloat16).double() @ w2.double().t(), rtol=1e-13, atol=1e-13)


def test_norm_reference_is_the_instance_norm_of_all_rows():
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(501, 48, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    gam, bet = torch.randn(48, generator=g) * 0.2 + 1.0, torch.randn(48, generator=g) * 0.3
    want = F.instance_norm(x.double().t()[None], weight=gam.double(), bias=bet.double(), eps=M.EPS)[0].t()
    assert torch.allclose(M.norm_ref(x, gam, bet), want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(M.norm_ref(x), F.instance_norm(x.double().t()[None], eps=M.EPS)[0].t(), rtol=1e-12, atol=1e-12)


def test_integer_case_stays_inside_its_exact_ranges():
    for C in (48, 96):
        c = M.int_case(333, C)
        for name, lo, hi in (("x", 0, 1), ("w1", -1, 1), ("w2", -1, 1), ("dy", -2, 2), ("res", -3, 3)):
            v = c[name].float()
            assert float(v.min()) == lo and float(v.max()) == hi and abs(float(v.mean()) - (lo + hi) / 2) > 0.05, name      # the whole set, off centre
        r = M.reference(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["res"], c["dy"])
        dx = M.assert_int_ranges(r, c["w1"])
        # the worst case of the construction, not only of this draw
        assert 128 - C >= 32 and 159 + C <= 255 and 4 * C * 255 + 76 + 3 < 2 ** 24 and 2 * C < 256 and 4 * C * 2 * C < 2 ** 24
        # a permuted fragment map changes the result: the rounded outputs are not symmetric under swapping channels
        assert not torch.equal(r["y"][:, :16], r["y"][:, 16:32]) and not torch.equal(dx[:16], dx[16:32])


def test_grid_arithmetic_of_every_row():
    ids = [i for i, _ in M.ROWS]
    assert len(set(ids)) == len(ids)
    for rid, kw in M.ROWS:
        C, m = kw["C"], kw["M"]
        assert f"-c{C}-" in rid and rid.endswith(f"-m{m}") and rid.startswith(kw["dir"] + "-")
        assert M.mtiles(m) == -(-m // 16) and M.blocks(m, C) == min(-(-M.mtiles(m) // 8), 512 if C == 48 else 256)
        w = M.walkers(m, C)
        assert w == max(0, M.mtiles(m) - 8 * M.blocks(m, C))      # (a grid below its cap has waves to spare: none walks)
        assert w == kw.get("walkers", 0), (rid, w)      # what the row states
        if "-walk-" in rid:
            assert w >= 3 and M.last_tile_rows(m) == 5 and M.blocks(m, C) == M.CAP[C], (rid, w)
        else:
            assert w == 0, (rid, w)
        assert M.last_tile_rows(m) == {4096: 16, 4101: 5}.get(m, 5)
        assert m >= 4096      # miseg_mlp_fused
    # the walk starts right above 16 rows x 8 waves x the cap
    for C in (48, 96):
        assert M.walkers(16 * 8 * M.CAP[C], C) == 0 and M.walkers(16 * 8 * M.CAP[C] + 1, C) == 1


def test_every_instantiation_is_named_by_a_launched_row():
    want = M.launcher_forms()
    assert len(want) == 12 and want == {("fwd", s, a, c) for s in (False, True) for a in (False, True) for c in (48, 96)} | {
        ("bwd", b, c) for b in (False, True) for c in (48, 96)}
    rows = {}
    for rid, kw in M.ROWS:
        rows.setdefault(M.form(kw), []).append(rid)
    assert set(rows) == want, want ^ set(rows)
    for f in want:      # each at full tiles and with a ragged last tile; each form that sums or normalises also walking
        ms = {kw["M"] for _, kw in M.ROWS if M.form(kw) == f}
        assert {4096, 4101} <= ms, (f, ms)
    walking = {M.form(kw) for rid, kw in M.ROWS if "-walk-" in rid}
    assert walking == {("fwd", True, a, c) for a in (False, True) for c in (48, 96)} | {("bwd", b, c) for b in (False, True) for c in (48, 96)}


def test_layout_rows_cover_every_view_and_the_table_matches_layouts_py():
    for d, views in M.VIEWS.items():
        for C in (48, 96):
            for lay in ("slice", "off8"):
                got = {next(iter(kw["lay"])) for _, kw in M.ROWS if kw["dir"] == d and kw["C"] == C and list(kw.get("lay", {}).values()) == [lay]}
                assert got == set(views), (d, C, lay, got)
            mixed = [kw for rid, kw in M.ROWS if kw["dir"] == d and kw["C"] == C and "-mixed-" in rid]
            assert len(mixed) == 1 and set(mixed[0]["lay"]) == set(views)
            lds = [ld for _, ld in mixed[0]["lay"].values()]
            assert len(set(lds)) == len(lds) and all(ld % 4 == 0 and off % 4 == 0 and off + M.view_cols(mixed[0])[o] <= ld
                                                     for o, (off, ld) in mixed[0]["lay"].items())
    for rid, kw in M.ROWS:      # a row only lays out views it passes
        assert set(kw.get("lay", {})) <= set(M.view_cols(kw)), rid
    assert M.layout(48, "slice") == (8, 72) and M.layout(48, "off8") == (4, 64) and M.layout(384, "ldodd") == (0, 393) and M.layout(96, (4, 104)) == (4, 104)


def test_refusal_table():
    ids = [r[0] for r in M.REFUSALS]
    assert len(set(ids)) == len(ids)
    from mi_seg_amd.hip import lib as L
    for m, C, hid, dt, yes in M.FUSED_EDGES:
        assert yes == int(dt == 1 and C in (48, 96) and hid == 4 * C and m >= 4096)
        assert L.load().miseg_mlp_fused(m, C, hid, dt) == yes      # (a host function: touches no device)
    for o in ("res", "dy", "dz", "h", "dx", "bs_x", "x", "y", "an_out"):
        assert any(r[2] == ("short", o) for r in M.REFUSALS), o
