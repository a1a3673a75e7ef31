"""The host-only plans of the instance-norm family (miseg_instnorm_{stats,apply,fwd,fwd_slabs,bwd,bwd_apply,bwd_slabs,bwd_reduce,pair_bwd}_plan;
csrc/norm.hip: norm_plan).  The launchers dispatch on them, so the kernel instantiation, lane width, thread geometry, grid and LDS bytes a
call reaches are pinned here without a card - what the GPU cases of tests/test_hip_instnorm_forms.py cannot show, because the card serves
unaligned 16-byte accesses.  The table is tests/instnorm_cases.py: hand-derived literal numbers, asked with stand-in addresses.  CPU only."""
import ctypes as C
import random

import pytest

import instnorm_cases as IC
import instnorm_ref as R


def _L():
    from mi_seg_amd.hip import lib
    return lib


@pytest.mark.parametrize("row", IC.ROWS, ids=lambda r: r["id"])
def test_the_plan_is_what_the_row_says(row):
    """return code, predicate and every launch; grid == (chunks, B, ctiles) or (ceil(cv / tx), B, 1); tx * ty <= 256; vec divides C"""
    L = _L()
    p, extra = IC.params(row, L)
    rc, pl = IC.ask(L, row["entry"], p, extra)
    IC.check_plan(row, L, rc, pl)
    if rc != IC.OK:
        assert pl.n_launches == 0 and bytes(pl) == bytes(C.sizeof(pl)), row["id"] + ": a refused plan is all zero"
        # the call itself refuses with the same code, on the host, before any launch (stream NULL; no device is touched)
        assert getattr(L.load(), IC.ENTRY_FN[row["entry"]])(C.byref(p) if p is not None else None, *extra, None) == rc, row["id"]


def test_a_null_plan_is_refused():
    L = _L()
    r = IC.BY_ID["stats-bf16-S2049-C24-tx3"]
    p, _ = IC.params(r, L)
    assert L.load().miseg_instnorm_stats_plan(C.byref(p), None) == IC.BADARG


def _reached(L):
    by_entry, inst = {fn: set() for fn in IC.ENTRY_FN.values()}, set()
    for r in IC.ROWS:
        for l in r["launches"]:
            by_entry[IC.ENTRY_FN[r["entry"]]].add(IC.kernel_id(L, l[0]))
            inst.add((l[0], r["dtype"], l[1], l[9]))
    return by_entry, inst


def test_every_kernel_of_every_entry_is_reached_by_a_row():
    L = _L()
    by_entry, _ = _reached(L)
    assert set(by_entry) == set(L.IN_KERNELS)
    for fn, kernels in L.IN_KERNELS.items():
        assert by_entry[fn] == set(kernels), f"{fn}: the table reaches {sorted(by_entry[fn])}, IN_KERNELS says {sorted(kernels)}"
    everything = {v for k, v in vars(L).items() if k.startswith("IN_") and isinstance(v, int)}
    assert everything == set().union(*L.IN_KERNELS.values()) | {L.IN_NONE} == set(range(10))


def test_every_instantiation_is_reached_or_listed_as_unreachable():
    L = _L()
    _, inst = _reached(L)
    every = IC.instantiations()
    assert inst <= every, f"rows name instantiations the launchers do not have: {sorted(inst - every)}"
    assert not (set(IC.UNREACHABLE) & inst), "an instantiation listed as unreachable is reached by a row"
    assert inst | set(IC.UNREACHABLE) == every, f"neither reached nor listed: {sorted(every - inst - set(IC.UNREACHABLE))}"


def test_the_generation_boundary_is_the_librarys_constant():
    assert _L().load().miseg_instnorm_fused_max_rows() == R.FUSED_MAX_ROWS == 2048


SWEEP_SEED = 20240611
SWEEP_CALLS = 4000


def test_seeded_sweep_every_accepted_plan_names_a_listed_instantiation():
    """random shapes, layouts and options through every entry point: an accepted plan has one or two launches of the entry's kernels, each a
    listed instantiation with a geometry whose every divisor is positive; a refused one is empty"""
    L = _L()
    rng = random.Random(SWEEP_SEED)
    every = IC.instantiations()
    accepted = refused = 0
    sizes = [1, 2, 15, 16, 17, 27, 255, 256, 257, 512, 513, 1000, 1024, 1025, 2047, 2048, 2049, 4096, 70000, 1 << 21]
    for i in range(SWEEP_CALLS):
        entry = rng.choice(sorted(IC.ENTRY_FN))
        dt = rng.choice(["bf16", "fp32"])
        S, Cc, B = rng.choice(sizes), rng.choice([1, 2, 3, 4, 6, 8, 10, 12, 13, 24, 40, 48, 50, 136, 256, 264, 320, rng.randrange(1, 400)]), rng.choice([1, 2, 3])
        lay = {o.rstrip("*"): rng.choice(["contig", "contig", "slice", "off8", "ldodd"]) for o in IC.OPERANDS[entry]}
        opts = {k: rng.random() < 0.5 for k in ("res", "act", "y", "dres", "gadd")}
        opts["rank1"] = entry in ("apply", "pair") and rng.random() < 0.3
        if entry.endswith("_slabs"):
            opts.update(nslabs=rng.choice([0, 1, 3]), gap=rng.choice([-1, 0, 6, 8]), slabs_off=rng.choice([0, 0, 8]))
        if rng.random() < 0.1:
            opts["set"] = rng.choice([{"num_styles": 0}, {"act": 2}, {"dtype": 5}, {"B": 0}, {"C": 0}, {"S": 0}])
        r = {"id": f"sweep{i}", "entry": entry, "dtype": dt, "B": B, "S": S, "C": Cc, "lay": lay, "opts": opts}
        p, extra = IC.params(r, L)
        rc, pl = IC.ask(L, entry, p, extra)
        what = f"{r}: rc {rc}"
        if rc != IC.OK:
            refused += 1
            assert rc in (IC.BADARG, IC.UNSUPPORTED) and pl.n_launches == 0, what
            continue
        accepted += 1
        assert pl.n_launches in (1, 2) and pl.aligned in (0, 1), what
        for l in list(pl.launch)[:pl.n_launches]:
            assert l.kernel in L.IN_KERNELS[IC.ENTRY_FN[entry]], what
        for t in IC.launches(L, pl):
            k, vec, cv, tx, ty, rpb, chunks, ctiles, lds, from_slabs, rank1 = t
            assert (k, dt, vec, from_slabs) in every, what
            assert vec >= 1 and cv >= 1 and tx >= 1 and ty >= 1 and tx * ty <= 256 and p.C % vec == 0 and cv * vec == p.C, what
            assert lds > 0 and lds <= 65536, what
            if k.startswith("FUSED") or k == "PAIR_FUSED_BWD":
                assert (rpb, chunks, ctiles) == (0, 0, 0) and p.S <= R.FUSED_MAX_ROWS and ty * 8 >= p.S, what
            else:
                assert rpb >= 1 and chunks >= 1 and ctiles >= 1 and chunks * rpb >= p.S and ctiles * tx >= cv, what
        for l in list(pl.launch)[:pl.n_launches]:
            assert min(l.grid_x, l.grid_y, l.grid_z) >= 1 and l.grid_y == p.B and l.threads == 256, what
    assert accepted > SWEEP_CALLS // 3 and refused > SWEEP_CALLS // 20, (accepted, refused)
