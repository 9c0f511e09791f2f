"""CPU checks of the weight-gradient matrix's reference side (tests/wgrad_reference.py): the exact family really is exact, the
emulation agrees with the float64 restatement, every planted defect is rejected by the verdict the GPU test uses, and the
matrix holds the edges it is meant to hold -- among them the split and tile regimes, from the restated launcher formulas."""
import pytest
import torch

import wgrad_reference as wr

SPECS = wr.matrix_specs()
WG = [s for s in SPECS if s["entry"] not in ("big", "ops_big")]
BIG = [s for s in SPECS if s["entry"] in ("big", "ops_big")]
_CASES = {}


def case_of(spec):
    if spec["id"] not in _CASES:
        _CASES[spec["id"]] = wr.build_case(spec)
    return _CASES[spec["id"]]


def of(entry, family="exact"):
    return [s for s in SPECS if s["entry"] == entry and s["family"] == family]


def test_ids_are_unique_and_name_the_case():
    ids = [s["id"] for s in SPECS]
    assert len(set(ids)) == len(ids)
    assert all(s["id"].startswith(s["entry"]) and "-R" in s["id"] and "-M" in s["id"] and "-N" in s["id"] for s in SPECS)


def test_exact_family_is_representable():
    """Every operand and masked operand is a bf16 value, every sum of magnitudes stays below 2^24 quarter units, and the same
    sums computed in float32 and in float64 have the same bits."""
    worst = 0.0
    for spec in WG:
        if spec["family"] != "exact":
            continue
        case = case_of(spec)
        for q, p in enumerate(case["probs"]):
            gh, xh, gm, src = wr.operands(p)
            for t in (p["g"], p["x"], gh, xh):
                assert torch.equal(wr.rne(t), t) and torch.equal(t * 4, (t * 4).round()) and float(t.abs().max()) <= 6.0
            assert float(p["g"].abs().max()) <= 3.0 and float(p["x"].abs().max()) <= 3.0
            assert gm is None or torch.equal(gm, gh)
            mag = gh.double().abs().t() @ xh.double().abs() + p["dw0"].double().abs()
            if p["bias"] is not None:
                mag = mag + p["bias"].double().abs()
            worst = max(worst, float(mag.max()) * 4)
            assert float(mag.max()) <= 36 * 2049 + 16
            dw32 = gh.t() @ xh + p["dw0"] + (p["bias"] if p["bias"] is not None else 0)
            assert torch.equal(dw32.double(), case_ref(case)[q]["dw"])
            if src is not None:
                assert torch.equal((src.sum(0) + p["db0"]).double(), src.double().sum(0) + p["db0"].double())
        if "hop" in case:
            h = case["hop"]
            assert all(float(t.abs().max()) <= 2 for t in h.values()) and 4 * max(256, 20 * 8) <= 2048      # fp16 holds every sum
        if "tail" in case:
            assert float(wr.tail_reference(case).abs().max()) < 2 ** 24
    assert worst < 2 ** 24
    for spec in BIG:
        for p in case_of(spec)["probs"]:
            assert torch.equal(wr.rne(p["g"]), p["g"]) and torch.equal(wr.rne(p["x"]), p["x"]) and 9 * p["R"] < 2 ** 24


def case_ref(case):
    wr.verdict(case, wr.emulate(case)) if "_ref" not in case else None
    return case["_ref"]


def test_emulation_agrees_with_the_reference():
    for spec in WG:
        case = case_of(spec)
        ok, ratio = wr.verdict(case, wr.emulate(case))
        assert ok and (ratio == 0.0 or spec["family"] == "round"), (spec["id"], ratio)
    for spec in BIG:
        case = case_of(spec)
        assert wr.big_verdict(case, wr.emulate(case)), spec["id"]


@pytest.mark.parametrize("mut", [m for m in wr.WGRAD_MUTANTS if m not in wr.ROUNDING_MUTANTS])
def test_exact_family_rejects(mut):
    """A bit mismatch on at least one exact case (and never a crash of the verdict on any)."""
    hits = [s["id"] for s in WG if s["family"] == "exact" and not wr.verdict(case_of(s), wr.emulate(case_of(s), mut))[0]]
    assert hits, mut


@pytest.mark.parametrize("mut,entries", [("truncate", ("plain", "masked", "mixed")), ("mask_after_round", ("masked",)),
                                         ("db_f32", ("plain", "masked", "mixed"))])
def test_rounding_family_rejects(mut, entries):
    """The rounding-related defects exceed `bound` on every entry point they can live in, at every R of the family -- by a wide
    margin: the bound of R <= 257 sits far below a truncating cast, a mask applied after rounding or column sums of the
    unrounded operand."""
    for entry in entries:
        for R in (9, 33, 257):
            ratios = [wr.verdict(case_of(s), wr.emulate(case_of(s), mut))[1] for s in of(entry, "round") if s["probs"][0]["R"] == R]
            print(f"{mut} {entry} R={R}: worst error / bound = {max(ratios):.1f}")
            assert max(ratios) > 2.0, (mut, entry, R, ratios)


def test_integers_cannot_see_the_rounding_defects():
    """... which is why the rounding family exists."""
    for mut in wr.ROUNDING_MUTANTS:
        assert all(wr.verdict(case_of(s), wr.emulate(case_of(s), mut))[0] for s in of("masked") + of("mixed"))


@pytest.mark.parametrize("mut", wr.BIG_MUTANTS)
def test_big_rejects(mut):
    assert [s["id"] for s in BIG if not wr.big_verdict(case_of(s), wr.emulate(case_of(s), mut))], mut


def test_masks_hold_both_zeros():
    for spec in WG:
        for p in case_of(spec)["probs"]:
            for m in (p["gmask"], p["xmask"]):
                if m is not None and m.numel() >= 4:
                    z = m[m == 0]
                    assert (m > 0).any() and (m < 0).any() and torch.signbit(z).any() and (~torch.signbit(z)).any()
                    f = wr.mask_factor(m, p["mask_vals"])
                    assert torch.equal(f[m == 0], torch.full_like(f[m == 0], p["mask_vals"][2]))


def test_matrix_holds_the_edges():
    def probs(entry, family="exact"):
        return [p for s in of(entry, family) for p in s["probs"]]
    for form in ("bf16", "f32"):
        got = {(p["R"], p["M"], p["N"]) for p in probs("plain") if p["form"] == form}
        assert {(R, M, N) for R in wr.PLAIN_R for (M, N) in wr.PLAIN_MN} <= got
    assert wr.PLAIN_R == (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 1537, 2049)
    assert wr.PLAIN_MN == ((2, 2), (6, 10), (30, 34), (32, 32), (34, 66), (130, 66))
    pl = probs("plain")
    assert {p["db"] for p in pl} == {None, "g"} and {p["view"] for p in pl} == {False, True}
    assert {(s["preload"], s["probs"][0]["db"]) for s in of("plain")} == {(a, b) for a in (False, True) for b in (None, "g")}
    # more tiles than the launcher's target: one split although the rows would allow more
    for R, M, target, slab in ((300, 736, 512, 256), (1100, 544, 256, 512)):
        s = next(s for s in of("plain") if s["probs"][0]["R"] == R and s["probs"][0]["M"] == M)
        nwave, tiles, splits, k = wr.regime(s)[0]
        assert tiles > target and splits == 1 and wr.cdiv(R, slab) > 1 and nwave * 32 == slab
    ma = probs("masked")
    assert {(p["gmask"], p["xmask"]) for p in ma} == {(True, False), (False, True), (True, True)}
    assert {p["db"] for p in ma} == {None, "g", "x"} and {p["R"] for p in ma} >= {1024, 1025}
    assert {(p["M"], p["N"]) for p in ma if p["gm_out"]} >= {(34, 10), (34, 66), (130, 66)}
    assert {s["preload"] for s in of("masked")} == {False, True}
    bi = of("bias")
    assert {p["form"] for s in bi for p in s["probs"]} == {"bf16", "f32"} and all(p["N"] % 32 for s in bi for p in s["probs"])
    for form in ("bf16", "f32"):
        sp = {wr.regime(s)[0][2] > 1 for s in bi if s["probs"][0]["form"] == form}
        assert sp == {False, True}
    assert any(wr.regime(s)[0][1] > 512 and wr.regime(s)[0][2] == 1 for s in bi)
    mi = probs("mixed")
    assert {(p["R"], p["db"]) for p in mi} == {(R, d) for R in (33, 1025) for d in (None, "x")}
    gr = of("group")
    assert {(len(s["probs"]), s["probs"][0]["R"], s["db_null_array"]) for s in gr} == \
        {(n, R, d) for n in (1, 4, 32) for R in (300, 1025) for d in (False, True)}
    assert any(any(p["db"] is None for p in s["probs"]) and any(p["db"] for p in s["probs"]) for s in gr)
    assert all(len({(p["M"], p["N"]) for p in s["probs"]}) == min(len(s["probs"]), 8) for s in gr)
    mu = of("multi")
    long_ = next(s for s in mu if s["tag"] == "long")
    assert {40, 1024, 1025, 2049} <= {p["R"] for p in long_["probs"]}
    assert all(r[0] == 16 for r in wr.regime(long_)) and all(r[0] == 8 for r in wr.regime(next(s for s in mu if s["tag"] == "short")))
    for s in (long_, next(s for s in mu if s["tag"] == "many16")):
        assert {p["form"] for p in s["probs"]} == {"bf16", "f32"} and {p["db"] for p in s["probs"]} == {None, "g", "x"}
        assert any(p["gmask"] or p["xmask"] for p in s["probs"]) and not all(p["gmask"] or p["xmask"] for p in s["probs"])
    assert len(next(s for s in mu if s["tag"] == "many16")["probs"]) == 32
    mh = of("multi_hop")
    assert {(s["hop"]["D"], s["hop"]["E"], s["hop"]["rt"]) for s in mh} == {(D, E, r) for D in (1, 3, 20) for E in (1, 5, 256) for r in (0, 1)}
    assert {wr.regime(s)[0][0] for s in mh} == {8, 16}
    ta = of("tail")
    assert {tuple(s["tail"].values()) for s in ta} == {(a, b, c) for a in (1, 33, 100) for b in (8, 40) for c in (32, 96)}
    assert all(p["R"] <= 1024 for s in ta for p in s["probs"]) and {len(s["probs"]) for s in ta} == {1, 4, 32}
    for entry in ("plain", "masked", "mixed"):
        assert {p["R"] for p in probs(entry, "round")} == {9, 33, 257}
    assert all(p["R"] <= 257 and p["form"] != "bf16" for s in SPECS if s["family"] == "round" for p in s["probs"])
    # some problem of the single-problem entries runs with several splits, some with one
    sp = {wr.regime(s)[0][2] > 1 for s in of("plain") + of("masked")}
    assert sp == {False, True}
    bg = of("big")
    assert {s["probs"][0]["R"] for s in bg} == {1, 63, 64, 65, 128, 129, 200}
    assert {(p["M"], p["N"]) for s in bg for p in s["probs"]} == {(m, n) for m in (8, 128, 136) for n in (8, 256, 264)}
    assert {len(s["probs"]) for s in bg} == {1, 2, 4} and {s["gview"] for s in bg} == {False, True}
    assert {s["S"] for s in bg} == {1, 2, "nchunk", "rec"}
    assert any(wr.big_S(s) == wr.cdiv(s["probs"][0]["R"], 64) > 1 for s in bg)                        # S == nchunk, several chunks
    assert any(wr.big_S(s) == 2 and wr.cdiv(s["probs"][0]["R"], 64) > 2 for s in bg)
    assert all(1 <= wr.big_S(s) <= wr.cdiv(s["probs"][0]["R"], 64) for s in bg)
    assert any(s["colsum"] is None for s in bg) and any(s["colsum"] == [0] and len(s["probs"]) > 1 for s in bg)
    assert any(s["colsum"] and len(s["probs"]) == 4 and s["colsum"] == [2] for s in bg)               # a middle job only
    assert any(s["preload"] and s["colsum"] for s in bg)
    assert [s for s in SPECS if s["entry"] == "ops_big"][0]["probs"][0]["R"] == 129


def test_restated_regimes():
    """fill_problem and the split recommendation, restated, at values worked out by hand from the sources."""
    assert wr.fill_problem(2432, 192, 192, 256, 16) == (36, 5, 512)          # the 5 splits csrc/wgrad.hip:203 reports
    assert wr.fill_problem(300, 6, 10, 512, 8) == (1, 2, 256)
    assert wr.fill_problem(1025, 34, 66, 256, 16) == (6, 3, 512)
    assert wr.fill_problem(31, 30, 34, 512, 8) == (2, 1, 256)
    assert wr.big_splits(12560, 24) == 10                                    # the S = 10 of csrc/wgradbig.hip:12
    assert wr.big_splits(129, 1) == 1 and wr.big_splits(200, 1) == 2 and wr.big_tiles(136, 264) == 4
    assert wr.big_ranges(200, 4) == [(0, 1), (1, 2), (2, 3), (3, 4)] and wr.big_ranges(129, 2) == [(0, 1), (1, 3)]


def test_big_regimes_from_the_library():
    """mobgt_layer_wgrad_big_tiles / _splits are host functions: the library's own answers for every big case of the matrix equal
    the restatement the emulation uses, the recommended S is legal, and the cases meant to run S == nchunk do.  (fill_problem is
    not exported: its restatement above cites the lines it comes from, and the exact GPU cases pass only if it is right about
    where `out_bias` and the splits fall.)"""
    from mobgt_amd import _lib
    _lib.build()
    lib = _lib.lib()
    for s in BIG:
        R = s["probs"][0]["R"]
        tiles = [lib.mobgt_layer_wgrad_big_tiles(p["M"], p["N"]) for p in s["probs"]]
        assert tiles == [wr.big_tiles(p["M"], p["N"]) for p in s["probs"]]
        rec = lib.mobgt_layer_wgrad_big_splits(R, sum(tiles))
        assert rec == wr.big_splits(R, sum(tiles)) and 1 <= rec <= wr.cdiv(R, wr.WB_KC)
        if s["S"] == "rec":
            assert wr.big_S(s) == rec
    assert {lib.mobgt_layer_wgrad_big_splits(s["probs"][0]["R"], 1) for s in BIG} >= {1, 2}
    assert lib.mobgt_layer_wgrad_big_splits(12560, 24) == 10 and lib.mobgt_layer_wgrad_big_tiles(768, 256) == 6
