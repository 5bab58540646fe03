"""CPU: the fp64 row-chain contract (tests/rowchain_contract.py) against itself — every case exercises the clauses it claims, the fp32 emulation of the
kernels' arithmetic passes every case at the bound derived from it, and those bounds are never looser than what tests/test_rowchain_gpu.py allows."""
import pytest
import torch

from tests import rowchain_contract as rc

ALL = [(e, n) for e in rc.CASES for n in rc.CASES[e]]
IDS = [f"{e}-{n}" for e, n in ALL]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("dname", list(rc.DTYPES))
@pytest.mark.parametrize("entry,name", ALL, ids=IDS)
def test_each_claimed_clause_moves_the_reference(entry, name, dname):
    """dropping a clause the case claims moves some output's rel-L2 by >= 4 x that output's bound on the case"""
    c, ref, emu, bnd = rc.case_data(entry, name, dname)
    cl = rc.claims(entry, c)
    assert set(cl) <= set(rc.CLAUSES[entry]) and set(rc.CLAUSES[entry]) <= set(rc.ABLATIONS)
    ratios = {}
    for clause in cl:
        ab = rc.reference(c, drop=(clause,))
        if clause == "vt_transpose":
            ab = {"vt": ab["vt"].reshape(ref["vt"].shape)}
        ratios[clause] = max(_rel(ab[o], ref[o]) / bnd[o][0] for o in ab)
    smallest = min(ratios.values()) if ratios else float("inf")
    print(f"{entry} {name} {dname}: emulation " + "; ".join(f"{o} rel-L2 {f[0]:.3e} worst block {f[1]:.3e} max-rel {f[2]:.3e}" for o, f in emu.items())
          + f"; smallest ablation / bound {smallest:.1f} ({min(ratios, key=ratios.get) if ratios else '-'})")
    assert all(v >= 4.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("entry", list(rc.CASES))
def test_every_clause_is_claimed_by_a_case(entry):
    claimed = set()
    for name, c in rc.CASES[entry].items():
        claimed |= set(rc.claims(entry, c))
    assert claimed == set(rc.CLAUSES[entry])


def test_unclaimed_switches_leave_the_reference_alone():
    """a switch outside an entry's clause list is no part of its reference (a typo in ``drop`` cannot pass for an ablation)"""
    c, ref, _, _ = rc.case_data("rc_linear", "m33_n64_ln", "bf16")
    assert torch.equal(rc.reference(c, drop=("key_pad", "item", "gn_coef"))["out"], ref["out"])


@pytest.mark.parametrize("dname", list(rc.DTYPES))
@pytest.mark.parametrize("entry,name", ALL, ids=IDS)
def test_emulation_passes_and_bounds_are_no_looser_than_before(entry, name, dname):
    c, ref, emu, bnd = rc.case_data(entry, name, dname)
    fails, fig = rc.judge(entry, c, rc.emulate(c), ref, bnd, f"{entry} {name} {dname}")
    assert not fails, fails
    for o, f in fig.items():
        assert all(x > 0 for x in f), (o, f)                   # a bound of 0 would ask for the fp64 result
    if c.get("peaked"):
        return                                                 # the peaked cases carry a bound of their own (see the module docstring of the GPU test)
    for o, (l2, _, mx) in bnd.items():
        old_l2, old_mx = rc.old_tolerance(entry, c, dname, o)
        print(f"{entry} {name} {dname} {o}: bound rel-L2 {l2:.3e} (old {old_l2:.3e}), max-rel {mx:.3e} (old {old_mx:.3e})")
        assert l2 <= old_l2 and mx <= old_mx


@pytest.mark.parametrize("dname", list(rc.DTYPES))
def test_emulation_folds_are_the_packers(dname):
    """``emulate`` uses W', u, v of the packers: the stream ``pack_xattn_q`` builds is ``rc_pack_tiles`` of the permuted rows of ``xattn_q_fold``"""
    from theatergen_amd import rowchain
    from theatergen_amd.weights_pack import rc_pack_tiles
    c, _, _, _ = rc.case_data("rc_xattn", "b1_r128_t0", dname)
    wp, u, v = rc.xattn_q_fold(c)
    perm = rowchain._q_slot_channels()
    want = rc_pack_tiles(wp[perm].contiguous(), v[perm], u[perm])
    assert torch.equal(rowchain.pack_xattn_q(c["wq"], None, c["gamma"], c["beta"], rc.DH ** -0.5), want)


def test_blocks_tile_every_output_once():
    for entry, name in ALL:
        c, ref, _, _ = rc.case_data(entry, name, "bf16")
        for o, ixs in rc.blocks(entry, c).items():
            cover = torch.zeros(ref[o].shape, dtype=torch.int32)
            for ix in ixs:
                cover[ix] += 1
            assert bool((cover == 1).all()), (entry, name, o)


def test_case_tables_hold_what_the_edges_need():
    lin = rc.LINEAR_CASES.values()
    assert {1, 31, 33, 255, 256, 257, 2050} <= {c["M"] for c in lin} and {64, 128, 320, 960} <= {c["N"] for c in lin}
    assert {(c["res"], bool(c["ln"])) for c in lin} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(c["dup"] and c["M"] % 32 for c in lin) and {(8.0, 0.125), (16.0, 0.0625)} <= {c["ln"][1:] for c in lin if c["ln"]}
    xa = rc.XATTN_CASES.values()
    assert {(1, 128), (3, 128), (17, 128), (1, 2176), (2, 384)} <= {(c["B"], c["rows"]) for c in xa} and {0, 4, 16} == {c["T"] for c in xa}
    assert {None, 0.0, 0.4, "item"} <= {c["ips"] for c in xa} and any(c["peaked"] and c["T"] == 16 for c in xa)
    s = rc.ip_scales(rc.XATTN_CASES["b17_r128_t16_item"])
    assert float(s.min()) < 0 and bool((s == 0).any()) and len(set(s[:5].tolist())) == 5
    assert {(1, 128), (3, 128), (17, 128), (1, 2176)} <= {(c["B"], c["rows"]) for c in rc.FRONT_CASES.values()}
    for e in rc.CASES:
        assert any(c["pitch"] for c in rc.CASES[e].values()) and any(not c["pitch"] for c in rc.CASES[e].values())
