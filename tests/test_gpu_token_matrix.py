"""The encoder-input kernels at every entry point and edge, through the C ABI (tests/token_abi.py), every case against the float64
reference of tests/token_reference.py: mobgt_token_fwd_chain, mobgt_token_bwd_chain, mobgt_assemble_tokens_fwd / _bwd / _qkv and
mobgt_embed_gather_multi on its own.

Each stage is judged on the device's OWN upstream output read back (f2 from the device's pt, nf from its x4, out from its nf / add,
qkv from its bf16 rows, dx4 from its d_nf, d_pt from its dx4), so a stage cannot hide behind the one in front of it.  Verdicts
(token_reference.judge_*): bit equality for the gathered rows, the assembly (an f32 restatement in the documented order), the bf16
copy, dropped elements, d_add / d_nf, the three entry points' `out` on identical operands, whole against split seeds, and every
guard row and column; the f32 products within (K + 2) 2^-24 (sum |a||w| + |b|) per element, qkv within one bf16 ulp of the reference
plus that bound, d_token and the scattered tables within (n + 2) 2^-24 sum |terms| of their initial value plus the float64 sum.
Nothing is fitted to a device's output; tests/test_host_token_reference.py shows on the CPU that these verdicts reject the mutants
of token_reference.MUTANTS.  The backward is fed the float64 forward's activations rounded to f32, with exact zeros planted on real
nodes.  A test id names entry point, G, N, padding family, dropout pair, seed mode and job layout (folds, additive tables, index type)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import token_abi as abi                                       # noqa: E402
import token_reference as tr                                  # noqa: E402
from mobgt_amd import _lib                                    # noqa: E402

DEV = "cuda"
SEED = 77
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def seeds(mode, seed=SEED):
    """(host seed, device word): the effective seed is their sum."""
    if mode == "split":
        return seed - 11, torch.tensor([11], dtype=torch.int64, device=DEV)
    return seed, None


def dev(t, dtype=F32):
    return t.to(dtype).to(DEV).contiguous()


def at_least_16_bytes(t, dtype=F32):
    """An operand on the device; an EMPTY one (N = 0) becomes a 16-byte dummy so that no null pointer goes in."""
    if t.numel():
        return dev(t, dtype)
    fill = tr.SENT if dtype.is_floating_point else int(tr.SENT)
    return torch.full((16 // torch.empty((), dtype=dtype).element_size(),), fill, dtype=dtype, device=DEV)


_W = {}


def weights(c):
    """Fuse weights and the packed QKV weight of a case on the device (kept for the last few cases)."""
    k = id(c)
    if k not in _W:
        if len(_W) > 4:
            _W.pop(next(iter(_W)))
        w = dict(token=dev(c.token), pe0=dev(c.pe0), keep=c)
        if c.C == tr.C_FUSED:
            w.update(w2=dev(c.w2), b2=dev(c.b2), w4=dev(c.w4), b4=dev(c.b4))
        if c.C in (192, 256):
            w.update(wq=abi.pack(dev(c.wq, BF)), bq=dev(c.bq, BF))
        _W[k] = w
    return {n: t for n, t in _W[k].items() if n != "keep"}


def job_dicts(c, idx_dtype, jobs=None):
    it = torch.int64 if idx_dtype == "i64" else torch.int32
    return [dict(table=dev(j.table), idx=at_least_16_bytes(j.idx, it), width=j.width, coff=j.coff, accum=j.accum, slot=j.slot, skip=j.skip)
            for j in (c.jobs if jobs is None else jobs)]


def idx_code(s):
    return abi.I64 if s["idx"] == "i64" else abi.I32


def forward_buffers(c, qkv=True, bf16=True, nodes=True):
    b = tr.Buffers(DEV)
    if nodes:
        b.add("pt", (c.R, c.W2))
        b.add("x4", (c.R, c.C))
        b.add("add", (c.R, c.C))
        b.add("nf", (c.R, c.C))
    b.add("out", (c.G * c.T, c.C))
    if bf16:
        b.add("out16", (c.G * c.T, c.C), BF)
    if qkv:
        b.add("qkv", (c.G * c.T, 3 * c.C), BF)
    return b


def run_fwd_chain(s, c, mode=None):
    i = dict(weights(c), real=at_least_16_bytes(c.real))
    b = forward_buffers(c)
    hs, sd = seeds(mode or s["seed_mode"])
    rc = abi.token_fwd_chain(job_dicts(c, s["idx"]), i, b.args(), c.G, c.N, idx_dtype=idx_code(s), slope2=c.slope2, slope4=c.slope4,
                             p_pos=c.p_pos, p_in=c.p_in, seed=hs, seed_dev=sd)
    _lib.check(rc, "mobgt_token_fwd_chain")
    torch.cuda.synchronize()
    return b


def run_assemble(entry, s, c, nf, add, bf16=True, mode=None):
    """mobgt_assemble_tokens_fwd / _qkv on the operands nf, add (device f32 tensors, or the case's own when None)."""
    i = dict(weights(c), real=at_least_16_bytes(c.real), nf=nf if nf is not None else at_least_16_bytes(c.nf_in),
             add=add if add is not None else at_least_16_bytes(c.add_in))
    b = forward_buffers(c, qkv=entry == "qkv", bf16=bf16, nodes=False)
    hs, sd = seeds(mode or s["seed_mode"])
    fn = abi.assemble_qkv if entry == "qkv" else abi.assemble_fwd
    _lib.check(fn(i, b.args(), c.G, c.N, c.C, c.p_pos, c.p_in, hs, sd), "mobgt_assemble_tokens_" + entry)
    torch.cuda.synchronize()
    return b, i


def no_failures(label, fails, b):
    fails = fails + b.guard_failures()
    assert not fails, (label, fails)


@pytest.mark.parametrize("spec", tr.fwd_specs(), ids=tr.spec_id)
def test_forward_chain(spec):
    s, c = spec, tr.cached_case(spec)
    b = run_fwd_chain(s, c)
    rep = {}
    fails = tr.judge_forward(c, b.cpu(), rep)
    print(tr.spec_id(s), "error / bound:", {k: "%.3f" % v for k, v in rep.items()})
    no_failures(tr.spec_id(s), fails, b)
    if c.R == 0:                                                   # the dropped `token + pe0` rows, whatever the node buffers hold
        want = tr.assemble_f32(c, torch.zeros(0, c.C), torch.zeros(0, c.C)).reshape(c.G, c.C)
        assert torch.equal(b.view["out"].cpu(), want)
    # the three entry points give identical `out` from identical nf / add
    nf, add = (b.view[n].contiguous() if c.R else None for n in ("nf", "add"))
    for entry in ("fwd", "qkv"):
        b2, _ = run_assemble(entry, s, c, nf, add)
        assert torch.equal(b2.view["out"], b.view["out"]) and torch.equal(b2.view["out16"], b.view["out16"]), entry
        no_failures(entry, [], b2)


@pytest.mark.parametrize("spec", [s for s in tr.fwd_specs() if s["drop"] != (0.0, 0.0) and s["seed_mode"] == "split"], ids=tr.spec_id)
def test_forward_whole_and_split_seeds_agree(spec):
    c = tr.cached_case(spec)
    a, b = run_fwd_chain(spec, c, "whole"), run_fwd_chain(spec, c, "split")
    for n in a.view:
        assert torch.equal(a.view[n], b.view[n]), n
    if c.R:                                                        # (and another seed does give another mask)
        other = tr.Buffers(DEV)
        other.add("out", (c.G * c.T, c.C))
        i = dict(weights(c), real=dev(c.real), nf=a.view["nf"].contiguous(), add=a.view["add"].contiguous())
        _lib.check(abi.assemble_fwd(i, other.view, c.G, c.N, c.C, c.p_pos, c.p_in, SEED + 1, None), "mobgt_assemble_tokens_fwd")
        assert not torch.equal(other.view["out"], a.view["out"])


def backward_inputs(s, c):
    y4, y2 = tr.saved_for_backward(c)
    ld_y2 = s["ld_y2"]
    hold = torch.full((c.R, ld_y2), 7.5, dtype=F32, device=DEV)                 # (ld 192: x4's leading columns, the category rows behind)
    hold[:, :c.W2] = dev(y2)
    i = dict(dout=dev(c.dout), real=dev(c.real), y4=dev(y4), y2=hold, w4=dev(c.w4), w2=dev(c.w2))
    return i, y4, y2


def backward_buffers(c, ld_dx4=None, chain=True):
    b = tr.Buffers(DEV)
    b.add("d_nf", (c.R, c.C))
    b.add("d_add", (c.R, c.C))
    if chain:
        b.add("dx4", (c.R, c.C), ld=ld_dx4)
        b.add("d_pt", (c.R, c.W2))
    b.add("d_token", (c.C,), fill=tr.TOKEN_INIT)
    return b


@pytest.mark.parametrize("spec", tr.bwd_specs(), ids=tr.spec_id)
def test_backward_chain(spec):
    s, c = spec, tr.cached_case(spec)
    i, y4, y2 = backward_inputs(s, c)
    outs = {}
    for mode in ("whole", "split") if (s["seed_mode"] == "split" and s["drop"] != (0.0, 0.0)) else (s["seed_mode"],):
        b = backward_buffers(c, s["ld_dx4"])
        hs, sd = seeds(mode)
        _lib.check(abi.token_bwd_chain(i, b.view, c.G, c.N, s["ld_y2"], s["ld_dx4"], slope4=c.slope4, slope2=c.slope2, p_pos=c.p_pos,
                                       p_in=c.p_in, seed=hs, seed_dev=sd), "mobgt_token_bwd_chain")
        torch.cuda.synchronize()
        rep = {}
        fails = tr.judge_backward(c, b.cpu(), y4, y2, report=rep)
        print(tr.spec_id(s), mode, "error / bound:", {k: "%.3f" % v for k, v in rep.items()})
        no_failures((tr.spec_id(s), mode), fails, b)
        outs[mode] = b
    if len(outs) == 2:
        for n in ("d_nf", "d_add", "dx4", "d_pt"):                 # (d_token: f32 atomics, not bitwise repeatable)
            assert torch.equal(outs["whole"].view[n], outs["split"].view[n]), n
    # mobgt_assemble_tokens_bwd gives the same d_nf / d_add
    b2 = backward_buffers(c, chain=False)
    hs, sd = seeds(s["seed_mode"])
    _lib.check(abi.assemble_bwd(i, b2.view, c.G, c.N, c.C, c.p_pos, c.p_in, hs, sd), "mobgt_assemble_tokens_bwd")
    torch.cuda.synchronize()
    no_failures("assemble_bwd", tr.judge_assembly_bwd(c, b2.cpu()), b2)
    for n in ("d_nf", "d_add"):
        assert torch.equal(b2.view[n], b.view[n]), n


@pytest.mark.parametrize("spec", tr.assemble_specs(), ids=tr.spec_id)
def test_assemble_entries(spec):
    s, c = spec, tr.cached_case(spec)
    entry = "qkv" if s["entry"] == "qkv" else "fwd"
    b, i = run_assemble(entry, s, c, None, None, bf16=s.get("bf16", "bf16") == "bf16")
    rep = {}
    nf, add = (c.nf_in.to(F32), c.add_in.to(F32))
    got = b.cpu()
    fails = tr.judge_assembly(c, got, nf, add, rep)
    no_failures(tr.spec_id(s), fails, b)
    if c.R == 0:
        for n in ("nf", "add", "real"):
            assert bool((i[n] == tr.SENT).all()), (n, "a dummy node buffer was touched")
    if entry == "qkv":
        b1, _ = run_assemble("fwd", s, c, None, None)
        assert torch.equal(b1.view["out"], b.view["out"]) and torch.equal(b1.view["out16"], b.view["out16"])
        return
    # ... and the backward of the same entry
    b2 = backward_buffers(c, chain=False)
    hs, sd = seeds(s["seed_mode"])
    ib = dict(dout=dev(c.dout), real=at_least_16_bytes(c.real))
    _lib.check(abi.assemble_bwd(ib, b2.args(), c.G, c.N, c.C, c.p_pos, c.p_in, hs, sd), "mobgt_assemble_tokens_bwd")
    torch.cuda.synchronize()
    no_failures(tr.spec_id(s) + " bwd", tr.judge_assembly_bwd(c, b2.cpu()), b2)


def gather_jobs_with_skips(c):
    """The case's jobs, each with a skip row that its index list does hold (where it holds a row at all)."""
    jobs = []
    for j in c.jobs:
        q = SimpleNamespace(**vars(j))
        rows = j.idx[j.idx >= 0]
        if j.accum != 2 and len(rows):
            q.skip = int(rows[len(rows) // 2])
        jobs.append(q)
    return jobs


@pytest.mark.parametrize("spec", tr.gather_specs(), ids=tr.spec_id)
def test_gather_multi_alone(spec):
    s, c = spec, tr.cached_case(spec)
    R, widths = c.R, tr.chain_widths(c)
    names = {0: "pt", 1: "x4", 2: "add"}
    # forward, with the folded tables; leading dimensions wider than the rows
    b = tr.Buffers(DEV)
    for slot, w in widths.items():
        b.add(names[slot], (R, w), ld=w + 8)
    jd = job_dicts(c, s["idx"])
    for j in jd:
        j["buf"], j["ld"] = b.view[names[j["slot"]]], b.full[names[j["slot"]]].stride(0)
    _lib.check(abi.gather_multi(jd, R, idx_code(s)), "mobgt_embed_gather_multi")
    torch.cuda.synchronize()
    no_failures(tr.spec_id(s), tr.judge_gather(c, b.cpu(), uncovered_zero=False), b)
    # backward: a skip row per table, extra_row0 on the positional job; then one table without a gradient and no extra row
    jobs = [j for j in gather_jobs_with_skips(c) if j.accum != 2]
    g = torch.Generator().manual_seed(R)
    bufs = {slot: torch.randn(R, w, generator=g, dtype=F32) for slot, w in widths.items()}
    extra = torch.randn(c.C, generator=g, dtype=F32)
    grads = tr.Buffers(DEV)
    for slot, w in widths.items():
        grads.add(names[slot], (R, w), ld=w + 4, fill=bufs[slot])
    pos = tr.live_index(c, c.pos_job)
    for no_grad, ex in (((), extra), ((1,), None)):
        t = tr.Buffers(DEV)
        jd = job_dicts(c, s["idx"], jobs)
        for k, (j, q) in enumerate(zip(jd, jobs)):
            j["buf"], j["ld"] = grads.view[names[j["slot"]]], grads.full[names[j["slot"]]].stride(0)
            j["d_table"] = t.add("t%d" % k, tuple(q.table.shape), fill=tr.TABLE_INIT) if k not in no_grad else None
        _lib.check(abi.gather_multi(jd, R, idx_code(s), backward=True, extra_row0=dev(ex) if ex is not None else None, extra_job=pos,
                                    tables=False), "mobgt_embed_gather_multi")
        torch.cuda.synchronize()
        got = [t.view["t%d" % k].cpu() if k not in no_grad else None for k in range(len(jobs))]
        fails = tr.judge_scatter(jobs, {k: v.to(F64) for k, v in bufs.items()}, got, extra_row0=ex.to(F64) if ex is not None else None,
                                 extra_job=pos, no_grad=no_grad)
        no_failures((tr.spec_id(s), "scatter", no_grad), fails, t)
        no_failures("the gradient buffers are inputs", [], grads)
        for k, q in enumerate(jobs):                                # a skipped row holds exactly what it held
            if k not in no_grad and q.skip >= 0 and not (ex is not None and k == pos and q.skip == 0):
                assert bool((got[k][q.skip] == tr.TABLE_INIT).all()), (k, "the skip row was written")


def test_refusals_return_without_launching():
    """What the header promises to refuse, as status codes; no output is touched."""
    s = tr._spec("fwd_chain", 2, 7, 0, pad="mixed", drop=(0.0, 0.0), layout="128+32", n_fold=1, n_add=4, idx="i64")
    c = tr.cached_case(s)
    w = dict(weights(c), real=dev(c.real))
    b = forward_buffers(c)
    o = b.view
    jobs = job_dicts(c, "i64")
    fwd = lambda jobs_=jobs, i=w, o_=o, **kw: abi.token_fwd_chain(jobs_, i, o_, kw.pop("G", c.G), kw.pop("N", c.N), **kw)      # noqa: E731
    no = lambda d, *ks: {k: v for k, v in d.items() if k not in ks}                                                              # noqa: E731
    edit = lambda k, **kw: [dict(j, **kw) if q == k else j for q, j in enumerate(jobs)]                                          # noqa: E731
    off4 = lambda t: t.data_ptr() + 4                                                                                           # noqa: E731
    slot = lambda n: [k for k, j in enumerate(jobs) if j["slot"] == n and j["accum"] != 2]                                       # noqa: E731
    folds = [k for k, j in enumerate(jobs) if j["accum"] == 2]
    assert folds and len(slot(0)) == 2 and len(slot(2)) >= 2, "the case must have a fold, two pt tables and several additive ones"
    E = abi.EBADDIM
    # ---- mobgt_token_fwd_chain
    assert fwd(C=256) == E and fwd(W2=128) == E and fwd(G=0) == E and fwd(N=-1) == E
    assert fwd(jobs[:2], n=2) == E                                                    # n < 3
    assert fwd(jobs + [dict(jobs[slot(1)[0]])]) == E                                  # two slot-1 jobs
    moved = [j for k, j in enumerate(jobs) if k not in folds]
    assert fwd(moved[:2] + [jobs[folds[0]]] + moved[2:]) == E                         # a fold behind the SECOND pt table
    assert fwd(moved[:3] + [jobs[folds[0]]] + moved[3:]) == E                         # ... behind the category table
    assert fwd(edit(folds[0], width=jobs[0]["width"] - 4)) == E                       # a fold of another width
    assert fwd(edit(slot(2)[1], coff=4)) == E                                         # slot 2 with coff != 0
    assert fwd(edit(slot(2)[0], accum=1)) == E                                        # a first slot-2 job that accumulates
    assert fwd(edit(slot(2)[1], accum=0)) == E                                        # ... and a later one that does not
    assert fwd(edit(slot(1)[0], width=30)) == E and fwd(edit(0, width=126)) == E      # a width that is no multiple of 4
    assert fwd(edit(slot(1)[0], coff=156)) == E                                       # the category row inside pt's columns
    for k in ("out16", "qkv", "pt", "x4", "add", "nf", "out"):
        assert fwd(o_=no(o, k)) == E, k
    for k in ("w2", "b2", "w4", "b4", "wq", "bq", "token", "pe0", "real"):
        assert fwd(i=no(w, k)) == E, k
    assert fwd(edit(slot(1)[0], idx=None)) == E
    i16 = [dict(j, idx=j["idx"].to(torch.int16)) for j in jobs]
    assert fwd(i16, idx_dtype=abi.I16) == abi.EDTYPE
    for k in ("w2", "w4", "wq"):
        assert fwd(i=dict(w, **{k: off4(w[k])})) == abi.EALIGN, k
    for k in ("qkv", "pt", "x4", "add", "nf"):
        assert fwd(o_=dict(o, **{k: off4(o[k])})) == abi.EALIGN, k
    assert fwd(edit(0, table=off4(jobs[0]["table"]))) == abi.EALIGN
    assert fwd(edit(folds[0], table=off4(jobs[folds[0]]["table"]))) == abi.EALIGN
    # ---- mobgt_assemble_tokens_fwd / _qkv / _bwd
    ia = dict(w, nf=dev(c.nf_in), add=dev(c.add_in))
    asm = lambda fn, i=ia, o_=o, G=c.G, N=c.N, C=c.C: fn(i, o_, G, N, C)                                                          # noqa: E731
    for fn in (abi.assemble_fwd, abi.assemble_qkv):
        assert asm(fn, G=0) == E and asm(fn, N=-1) == E
        for k in ("nf", "real", "add", "token", "pe0"):
            assert asm(fn, i=no(ia, k)) == E, k
        assert asm(fn, o_=no(o, "out")) == E
    assert asm(abi.assemble_fwd, C=0) == E
    assert asm(abi.assemble_qkv, C=128) == E and asm(abi.assemble_qkv, C=190) == E
    for k in ("wq", "bq"):
        assert asm(abi.assemble_qkv, i=no(ia, k)) == E, k
    for k in ("out16", "qkv"):
        assert asm(abi.assemble_qkv, o_=no(o, k)) == E, k
    assert asm(abi.assemble_qkv, i=dict(ia, wq=off4(w["wq"]))) == abi.EALIGN
    assert asm(abi.assemble_qkv, o_=dict(o, qkv=off4(o["qkv"]))) == abi.EALIGN
    sb = dict(s, ld_y2=160, ld_dx4=192)
    ib, _, _ = backward_inputs(sb, c)
    bb = backward_buffers(c, 192)
    ob = bb.view
    assert abi.assemble_bwd(ib, ob, 0, c.N, c.C) == E and abi.assemble_bwd(ib, ob, c.G, -1, c.C) == E
    for k in ("dout", "real"):
        assert abi.assemble_bwd(no(ib, k), ob, c.G, c.N, c.C) == E, k
    for k in ("d_nf", "d_add", "d_token"):
        assert abi.assemble_bwd(ib, no(ob, k), c.G, c.N, c.C) == E, k
    # ---- mobgt_token_bwd_chain
    bwd = lambda i=ib, o_=ob, G=c.G, N=c.N, ld_y2=160, ld_dx4=192, **kw: abi.token_bwd_chain(i, o_, G, N, ld_y2, ld_dx4, **kw)  # noqa: E731
    assert bwd(G=0) == E and bwd(N=0) == E and bwd(C=256) == E and bwd(W2=128) == E
    assert bwd(ld_y2=156) == E and bwd(ld_dx4=188) == E
    for k in ib:
        assert bwd(i=no(ib, k)) == E, k
    for k in ob:
        assert bwd(o_=no(ob, k)) == E, k
    for k in ("w4", "w2"):
        assert bwd(i=dict(ib, **{k: off4(ib[k])})) == abi.EALIGN, k
    # ---- mobgt_embed_gather_multi
    gb = tr.Buffers(DEV)
    names = {0: "pt", 1: "x4", 2: "add"}
    for slot_, wd in tr.chain_widths(c).items():
        gb.add(names[slot_], (c.R, wd))
    gj = [dict(j, buf=gb.view[names[j["slot"]]], ld=gb.view[names[j["slot"]]].stride(0)) for j in jobs]
    gat = lambda jobs_=gj, **kw: abi.gather_multi(jobs_, c.R, **kw)                                                              # noqa: E731
    extra = dev(c.token)
    assert gat(extra_row0=extra, extra_job=len(gj) - 1) == E                          # extra_row0 in a forward call
    live = [j for j in gj if j["accum"] != 2]
    assert gat(live, backward=True, extra_row0=extra, extra_job=len(live)) == E       # ... for a job that is not there
    assert gat(gj, backward=True) == E                                                # a folded table in a backward call
    assert gat([gj[folds[0]]] + gj) == E                                              # a fold with nothing in front of it
    assert gat([dict(j, table=None) if k == 0 else j for k, j in enumerate(gj)]) == E
    assert gat([dict(j, idx=None) if k == 0 else j for k, j in enumerate(gj)]) == E
    assert gat([dict(j, buf=None) if k == 0 else j for k, j in enumerate(gj)]) == E
    assert gat([dict(j, width=30) if k == 0 else j for k, j in enumerate(gj)]) == E
    assert gat(gj * 2) == E                                                           # more than 8 jobs + 3 folds
    assert gat(idx_dtype=abi.I16) == abi.EDTYPE
    assert gat([dict(j, table=off4(j["table"])) if k == 0 else j for k, j in enumerate(gj)]) == abi.EALIGN
    assert gat([dict(j, buf=off4(j["buf"])) if k == 0 else j for k, j in enumerate(gj)]) == abi.EALIGN
    torch.cuda.synchronize()
    for label, bufs in (("forward", b), ("backward", bb), ("gather", gb)):
        for n, full in bufs.full.items():
            v = bufs.view[n]
            assert bool(torch.isnan(v).all()) or n == "d_token", (label, n, "a refused call wrote")
        no_failures(label, [], bufs)
    assert bool((bb.view["d_token"] == tr.TOKEN_INIT).all())
