"""tests/chain_reference.py without a GPU: the float64 emulation of the chain kernels' rounding points stays within its stated budget of
the float64 autograd reference, its hand-written backward IS the reference once rounding is switched off, the tolerances the GPU
matrix forms from it (tests/test_gpu_chain_matrix.py) reject every deliberately wrong computation and accept the right one, the
row-floor condition holds for every input family, and the matrix covers what it claims."""
import pytest
import torch

import chain_reference as cr

# Budget of the emulation against the reference: each bf16 rounding point contributes 2^-9 relative per element (2^-9 / sqrt(3) rms);
# a tensor sits behind at most nine of them along the chain (a .. qkv forward, dout .. da backward), which add in quadrature to
# 3 x 2^-9 over a row and reach about twice that in a single element: 2^-7 per row and whole tensor, and the ceiling of the
# existing chain tests for an element.  The common-mode and flat-row families are exempt from the ceilings, not from this budget's form:
# their rows carry a mean (or an rstd) two orders above the signal, so they get 2^-4.
BUDGET = {"row": 2.0 ** -7, "l2": 2.0 ** -7, "elem": cr.CAP_ELEM}
BUDGET_UNCAPPED = {"row": 2.0 ** -4, "l2": 2.0 ** -4, "elem": 2.0 ** -4}
KINDS = {"post": dict(tail=True), "post_last": dict(last=True), "preln": dict(preln=True, tail=True),
         "preln_alone": dict(preln=True, successor=False, last=True)}


def all_names(c):
    return cr.fwd_names(c) + cr.bwd_names(c, big=True) + ["dz"]


def case_for(family, kind, R=33, p=0.1, **kw):
    args = dict(KINDS[kind])
    args.update(kw)
    return cr.make_case(128 if "preln" in kind else 192, R, family, p_drop=p, **args)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("family", cr.FAMILIES)
def test_emulation_within_its_rounding_budget(family, kind):
    c = case_for(family, kind, n_wg=2)
    ref = cr.case_reference(c)
    budget = BUDGET_UNCAPPED if family in cr.UNCAPPED else BUDGET
    for n_split in (1, 4, 3):
        emu = cr.case_emulation(c, n_split)
        for name in all_names(c):
            m = cr.measure(emu[name], ref[name])
            for k, lim in budget.items():
                assert m[k] <= lim, (family, kind, n_split, name, k, m[k], lim)
    tol = cr.tolerances(c, all_names(c))
    if family not in cr.UNCAPPED:
        for name, t in tol.items():
            cap = {"fwd": cr.CAP_ELEM, "bwd_rows": cr.CAP_BWD_ROWS, "sums": cr.CAP_SUMS}[cr.kind_of(name)]
            assert t["elem"] <= cap and t["l2"] <= cr.CAP_ELEM
            assert 2.0 * t["emu"]["elem"] <= cap, "the family's parameters are wrong: the emulation alone reaches the ceiling"


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("family", cr.FAMILIES)
def test_hand_written_backward_is_autograd_without_rounding(family, kind):
    c = case_for(family, kind, n_wg=1)
    ref = cr.reference(c)
    for n_split in (1, 2, 3):
        got = cr.emulation(c, rounding=False, n_split=n_split)
        for name in all_names(c):
            m = cr.measure(got[name], ref[name])
            assert max(m["row"], m["l2"], m["elem"]) <= 1e-11, (family, kind, name, m)


@pytest.mark.parametrize("kind", ["post", "preln"])
@pytest.mark.parametrize("R", [1, 15, 33, 65, 333])
@pytest.mark.parametrize("family", cr.FAMILIES)
def test_floor_share_condition(family, kind, R):
    """At most FLOOR_SHARE_CAP of the judged rows of any tensor lie under the row floor, in the float64 reference alone."""
    c = case_for(family, kind, R=R)
    for name, share in cr.floor_shares(c).items():
        assert share <= cr.FLOOR_SHARE_CAP, (family, kind, R, name, share)
    if family == "sparse" and R > 2:
        ref = cr.case_reference(c)
        zero = [r for r in range(R) if r not in c.nonzero]
        for name in ("df", "du", "dy", "da", "dx1"):
            assert float(ref[name][zero].abs().max()) == 0.0 and cr.measure(ref[name], ref[name])["n_zero"] == len(zero)


# mutant -> the case of the GPU matrix that must catch it (family, kind, R, extra)
MUTANT_CASES = {
    "no_inv_keep_site2": [("plain", "post", 33, {}), ("plain", "preln", 17, {})],
    "site2_mask_of_site1": [("plain", "post", 33, {}), ("gelu", "preln", 65, {})],
    "ln_bwd_without_xhat_term": [("plain", "post", 33, {}), ("common", "post", 33, {}), ("dom_y", "preln", 33, {})],
    # (on N(0, 1) rows a bf16-rounded input moves the mean by 2^-9 / sqrt(C) of a row: under one rounding point -- the common-mode family is its case)
    "ln_stats_from_bf16": [("common", "post", 33, {}), ("common", "preln", 65, {})],
    "w2_kstep_missing": [("plain", "post", 33, {}), ("gelu", "post", 17, {})],
    "colsum_full_blocks_only": [("plain", "post", 33, {}), ("sparse", "post", 15, {}), ("plain", "preln", 65, {})],
    "tail_behind_the_norm": [("plain", "post", 33, {}), ("dom_x", "post", 17, {})],
    "gelu_grad_of_h": [("plain", "post", 33, {}), ("gelu", "post", 33, {})],
    "dw_last_split_skipped": [("plain", "preln", 1040, dict(n_wg=2)), ("plain", "preln", 1040, dict(n_wg=4))]    # (C = 128: the [C, C] problem has 16 tiles and 3 splits),
}


def test_every_mutant_has_a_case():
    assert set(MUTANT_CASES) == set(cr.MUTANTS)


@pytest.mark.parametrize("which", cr.MUTANTS)
def test_mutants_are_rejected_and_the_reference_is_accepted(which):
    for family, kind, R, extra in MUTANT_CASES[which]:
        c = case_for(family, kind, R=R, **extra)
        ref = cr.case_reference(c)
        for n_split in (1, 3):
            tol = cr.tolerances(c, cr.fwd_names(c) + cr.bwd_names(c, big=True), n_split)
            assert not cr.compare(ref, ref, tol)["fail"]
            assert not cr.compare(cr.emulation(c, rounding=False), ref, tol)["fail"]
            assert not cr.compare(cr.case_emulation(c, n_split), ref, tol)["fail"]
            bad = cr.mutant(c, which)
            assert bad is not None, (which, family, kind, R)
            rep = cr.compare(bad, ref, tol)
            assert rep["fail"], (which, family, kind, R, n_split)
            assert cr.worst_ratio(rep, tol) >= 1.5, (which, family, kind, R, cr.worst_ratio(rep, tol))


def test_mutants_that_do_not_apply_return_none():
    c = cr.make_case(192, 32, "plain")
    for which in ("no_inv_keep_site2", "site2_mask_of_site1", "colsum_full_blocks_only", "tail_behind_the_norm", "dw_last_split_skipped"):
        assert cr.mutant(c, which) is None


def test_passenger_split_rule():
    # csrc/wgrad_body.h fill_problem: 64 workgroups aimed at, slabs of 384 rows
    assert cr.passenger_last_split(33, 128, 128) == 33                     # one split
    assert cr.passenger_last_split(1040, 128, 128) == 768                  # 16 tiles: min(4, 3) = 3 splits of 384
    assert cr.passenger_last_split(1040, 384, 128) == 1040                 # 48 tiles: one split
    assert cr.passenger_last_split(1040, 1024, 128) == 1040


def test_inv_keep_and_masks():
    assert cr.inv_keep_of(0.0) == 1.0
    assert abs(cr.inv_keep_of(0.1) - 1.0 / (1.0 - 6554 / 65536.0)) < 1e-7
    c = cr.make_case(128, 65, "plain", p_drop=0.1)
    assert abs(1.0 - float(c.keep1.mean()) - 0.1) < 0.02 and not torch.equal(c.keep1, c.keep2)


def test_matrix_covers_its_table():
    """Every row of the dispatch matrix is in the ids, and the pairwise thinning keeps every pair it promises."""
    specs = cr.matrix_specs(256)
    ids = [cr.spec_id(s, 256) for s in specs]
    assert len(set(ids)) == len(ids)
    have = lambda **kw: any(all(s[k] == v for k, v in kw.items()) for s in specs)       # noqa: E731
    for C in (128, 192, 256):
        for form in ("one", "cl4", "cl2", "big64"):
            for d in ("fwd", "bwd"):
                assert have(C=C, form=form, dir=d), (C, form, d)
        assert have(C=C, form="bwd_big", dir="bwd")
    for R in (1, 15, 16, 17, 33, 63, 64, 65, 4096, 4097, 4150, 4160):
        assert have(R=R, dir="fwd") and have(R=R, dir="bwd"), R
    for form in ("one", "cl4", "cl2", "big64", "bwd_big"):
        for fam in cr.FAMILIES:
            assert have(form=form, family=fam), (form, fam)
        for p, mode in ((0.0, "host"), (0.1, "host"), (0.1, "split")):
            assert have(form=form, p=p, seed_mode=mode), (form, p, mode)
    for succ in (True, False):
        assert have(preln=True, successor=succ, dir="fwd", C=128)
    for tail in (True, False):
        assert have(preln=True, tail=tail, dir="bwd") and have(preln=False, tail=tail, dir="bwd")
    assert have(last=True, dir="fwd", preln=False)
    for n_wg in (0, 1, 4):
        assert have(n_wg=n_wg, dir="bwd")
    assert have(n_wg=4, with_db=False) and have(n_wg=4, with_db=True) and have(n_wg=1, preln=True)
    assert have(form="bwd_big", R=33) and have(form="bwd_big", R=4150)
    for form in ("one", "cl4", "cl2", "big64"):
        assert have(form=form, dir="both")
