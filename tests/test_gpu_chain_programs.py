"""Seeded random programs (tests/chain_programs.py) through the chain compiler on the GPU, at both word lengths: every program of the seed
set over every branch of csrc/chain.inc's chain_batch() / rest_of() / chain_aos() and of its two IO objects, compared with

  * the call-by-call sequence through Field(P, wl) (run_calls) with torch.equal: element words, int32 arrays, byte records;
  * on X25519, NIST256 and X448 at 64 bits the CPU oracle, operation by operation on the reference's own rows (run_oracle): word for
    word, byte for byte, int for int -- a truth that shares no code with any kernel (values of limb_free(), whose limbs are those of the
    library's own addition chains, after redc);
  * the integer model (run_model) wherever it is determined.

Operands, truths and plug-ins are made once per case; every shape below is a prefix of the same pool.  Shapes are the smallest that reach
each branch: n = 1; two workgroups of lanes at the widest width plus 3 in aligned rows (a ragged tail and a remainder launch); a row
stride that forces the next narrower width; tiles of 128; element arrays one word off 16-byte alignment and record arrays 8 bytes off
it (one element per lane, the direct path); outputs in the arrays of inputs (the three aliasings docs/fused_chains.md allows); one
512-element chunk plus 5 through the element-major entry."""
import os

import pytest

from tests import chain_programs as cp
from tests.test_gpu_fuse_bytes import _at, _misaligned
from tests.test_gpu_fuse_le import _tiled_like
from tests.test_gpu_fuse_shared import _bcast, _dev

pytestmark = pytest.mark.gpu
BLOCK = 256                                                      # workgroup size of a chain at either word length
PATHS = ("staged", "direct")
AOS_N = 512 + 5                                                  # one chunk of the element-major kernel and 5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


class Prog:
    pass


def _flat_n(ept):
    return 2 * BLOCK * ept + 3


def _prepare(torch, F, oracle, P, wl, built, profile, seed):
    """one program: its builds, its operands on the host and on the device, and the three truths over the whole pool"""
    g = Prog()
    g.f = built[(profile, seed, None)]
    g.wide = {e: built[(profile, seed, e)] for e in (2, 4) if (profile, seed, e) in built}
    g.ch, g.profile = g.f.chain, profile
    g.runs, g.differs = 0, []                                    # 'unreduced': runs compared with the call sequence, and those that differed
    ch = g.ch
    g.ept = 1 if ch._long() else 2 if wl == 64 else 1
    g.n0 = max(_flat_n(max([g.ept] + list(g.wide))), AOS_N)
    g.data = rows, shared, sels, records = cp.make_batch(ch, g.n0, seed)
    g.elems = [_dev(torch, wl, r) for r in rows]
    g.shared = shared
    g.sels = [torch.tensor(d, dtype=torch.int32, device="cuda") for d in sels]
    g.recs = [torch.tensor([list(r) for r in col], dtype=torch.uint8, device="cuda") for col in records]
    like = g.elems[0] if g.elems else F.empty(g.n0)
    g.calls = cp.run_calls(ch, F, [x.clone() for x in g.elems], [_bcast(torch, wl, b, like) for b in shared], [d.clone() for d in g.sels], [r.clone() for r in g.recs])
    g.free = cp.limb_free(ch)
    g.oracle = None
    if wl == 64 and P in cp.ORACLE_PRIMES:
        E, B, I = cp.run_oracle(ch, oracle, *g.data)
        g.oracle = ([_dev(torch, wl, col) for col in E], [torch.tensor([list(r) for r in col], dtype=torch.uint8, device="cuda") for col in B],
                    [torch.tensor(col, dtype=torch.int32, device="cuda") for col in I])
    g.model = cp.run_model(ch, cp.fp_of(P, wl), *g.data)
    return g


@pytest.fixture(scope="module", params=cp.CASES, ids=lambda c: "%s-w%d" % c)
def ctx(request, torch_cuda, oracle):
    from modarith_amd import generate as gen
    from modarith_amd.field import Field
    P, wl = request.param
    if P == cp.GENERATED and gen.find_field(P, wl=64, built=True) is None:
        pytest.skip("no plug-in of the generated field %s in this tree" % P)
    # independent hipcc units, seconds each: those of every case side by side through one pool, the first time round
    built = cp.build_all(cp.available_cases(), workers=min(16, len(os.sched_getaffinity(0))))[(P, wl)]
    mp = pytest.MonkeyPatch()
    mp.delenv("MA_CHAIN_BYTES", raising=False)                   # (the truths below are made on the shipped byte path)
    F = Field(P, wl=wl, tile=None)
    yield P, wl, F, [_prepare(torch_cuda, F, oracle, P, wl, built, pr, s) for pr, s in cp.programs(P, wl)]
    mp.undo()


# ---------------------------------------------------------------------------------------------------------------- one call and its checks
def _compare(torch, F, g, got, lo, n, what):
    """the outputs of a call on elements lo .. lo + n - 1 of the pool against the truths"""
    ch = g.ch
    ne, nb = len(ch.outs), len(ch.bouts)
    E, B, I = got[:ne], got[ne:ne + nb], got[ne + nb:]
    cut = lambda t: t[..., lo:lo + n] if t.dim() == 2 and t.dtype != torch.uint8 else t[lo:lo + n]
    same = all(torch.equal(F.to_flat(x), cut(w)) for x, w in zip(E, g.calls[0])) and all(torch.equal(x, cut(w)) for x, w in zip(B, g.calls[1])) \
        and all(torch.equal(x, cut(w)) for x, w in zip(I, g.calls[2]))
    if g.profile == "unreduced":                                 # the oracle alone is the truth here; that the calls agree with it is a claim of
        g.runs += 1                                              # docs/fused_chains.md with a test of its own, the last of this module
        if not same:
            g.differs.append(what)
    else:
        assert same, (ch.name, what, "call by call")
    if g.oracle is not None:
        for k, (x, w) in enumerate(zip(E, g.oracle[0])):
            x = F.to_flat(x).contiguous()
            if ch.outs[k] in g.free:
                x = F.redc(x)
            assert torch.equal(x, cut(w)), (ch.name, what, "oracle, element output %d" % k)
        for k, (x, w) in enumerate(zip(B, g.oracle[1])):
            assert torch.equal(x, cut(w)), (ch.name, what, "oracle, byte output %d" % k)
        for k, (x, w) in enumerate(zip(I, g.oracle[2])):
            assert torch.equal(x, cut(w)), (ch.name, what, "oracle, int output %d" % k)


def _against_the_model(torch, F, g, got, n):
    ch, fp = g.ch, cp.fp_of(g.ch.prime, g.ch.wl)
    ne, nb = len(ch.outs), len(ch.bouts)
    ME, MB, MI = g.model
    for k, x in enumerate(got[:ne]):
        free = ch.outs[k] in g.free
        x = F.to_flat(x).contiguous()
        rows = F.to_limbs(F.redc(x) if free else x)
        mask = (1 << ch.wl) - 1
        for j in range(n):
            assert cp.model_agrees(fp, ME[k][j], [int(v) & mask for v in rows[j]], free) is not False, (ch.name, "model, element output %d" % k, j)
    for k, x in enumerate(got[ne:ne + nb]):
        rows = x.cpu().numpy()
        for j in range(n):
            assert MB[k][j] is None or MB[k][j] == bytes(rows[j]), (ch.name, "model, byte output %d" % k, j)
    for k, x in enumerate(got[ne + nb:]):
        col = x.cpu().tolist()
        for j in range(n):
            assert MI[k][j] is None or MI[k][j] == col[j], (ch.name, "model, int output %d" % k, j)


def _inputs(torch, F, g, n, width=None, lo=0, tile=None, off=False):
    """the call's element batches (rows of `width` words; tiled; or one word off 16-byte alignment), records (8 bytes off it) and selectors"""
    wl = g.ch.wl
    elems = []
    for x in g.elems:
        x = x[:, lo:lo + n].contiguous()
        if tile:
            x = F.to_tiled(x, tile)
        elif off:
            x = _misaligned(torch, x, wl)
        elif width:
            big = torch.zeros((x.shape[0], width), dtype=x.dtype, device="cuda")
            big[:, :n] = x
            x = big[:, :n]
        elems.append(x)
    recs = [(_at(torch, r[lo:lo + n], 8) if off else r[lo:lo + n].clone()) for r in g.recs]
    return elems, recs, [d[lo:lo + n].clone() for d in g.sels]


def _run(torch, F, g, f, n, what, out=None, aliased=(), **shape):
    elems, recs, sels = _inputs(torch, F, g, n, **shape)
    before = [t.clone() for t in elems + recs + sels]
    got = f(*elems, *recs, *g.shared, *sels, out=out(elems, recs, sels) if out else None)
    _compare(torch, F, g, got, shape.get("lo", 0), n, what)
    for k, (t, b) in enumerate(zip(elems + recs + sels, before)):
        if not any(t is a for a in aliased):
            assert torch.equal(t, b), (g.ch.name, what, "input %d changed" % k)
    return got, (elems, recs, sels)


def _paths(g):
    return PATHS if g.ch.bins or g.ch.bouts else (None,)


def _set(monkeypatch, path):
    if path is None:
        monkeypatch.delenv("MA_CHAIN_BYTES", raising=False)
    else:
        monkeypatch.setenv("MA_CHAIN_BYTES", path)


# ---------------------------------------------------------------------------------------------------------------- tests
def test_flat_batches(ctx, torch_cuda, monkeypatch):
    """two workgroups of lanes at the build's width plus 3, in aligned rows: the main launch with a ragged last workgroup and the
    remainder launch; n = 1; the model on the first of them"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    for g in progs:
        for path in _paths(g):
            _set(monkeypatch, path)
            n = _flat_n(g.ept)
            got, (elems, _, _) = _run(torch, F, g, g.f, n, ("flat", path), width=n + 1)
            assert all(x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0 for x in elems)
            _against_the_model(torch, F, g, got, n)
            _run(torch, F, g, g.f, 1, ("n = 1", path))
            _run(torch, F, g, g.f, 1, ("n = 1, last of the pool", path), lo=g.n0 - 1)


def test_the_model_over_the_whole_pool(ctx, torch_cuda):
    """every run of this module is compared with the call-by-call results over the pool with torch.equal (_compare); those results agree
    with the model wherever it is determined, on every element of the pool -- the ones only the wider builds reach included --, so every
    run does.  Where there is no oracle (32 bits, 2519) this is the truth that shares no code with Field<P>.  The 'unreduced' programs,
    whose runs are not held to the call sequence, meet the model through their flat runs (test_flat_batches)"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    for g in progs:
        _against_the_model(torch, F, g, list(g.calls[0]) + list(g.calls[1]) + list(g.calls[2]), g.n0)


def test_tiles_and_the_next_narrower_width(ctx, torch_cuda, monkeypatch):
    """tiles of 128; rows whose stride is no multiple of the build's width, so that the call drops to half of it"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    for g in progs:
        for path in _paths(g):
            _set(monkeypatch, path)
            if g.ch.nin or g.ch.outs:
                n = 384
                out = None
                if not g.ch.nin:                                 # element results of byte records alone: the caller says that they are tiled
                    out = lambda e, r, s: ([_tiled_like(torch, F, n, 128) for _ in g.ch.outs] + [torch.empty((n, F.nbytes), dtype=torch.uint8, device="cuda") for _ in g.ch.bouts]
                                           + [torch.empty(n, dtype=torch.int32, device="cuda") for _ in g.ch.pouts])
                _run(torch, F, g, g.f, n, ("tiles of 128", path), tile=128, out=out)
            for f, e in [(g.f, g.ept)] + [(f, e) for e, f in g.wide.items()]:
                if e > 1 and g.ch.nin:
                    n = _flat_n(e)
                    _run(torch, F, g, f, n, ("stride %d mod %d" % (e // 2, e), path), width=n + 1 + e // 2)


def test_misaligned_arrays(ctx, torch_cuda, monkeypatch):
    """element arrays one word behind a 16-byte boundary: one element per lane whatever the build; record arrays 8 bytes behind one: the
    direct path whatever was asked for"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    for g in progs:
        for path in _paths(g):
            _set(monkeypatch, path)
            for f in [g.f] + list(g.wide.values()):
                n = BLOCK + 5
                _, (elems, recs, _) = _run(torch, F, g, f, n, ("misaligned", path), off=True)
                assert all(x.data_ptr() % 16 == wl // 8 for x in elems) and all(r.data_ptr() % 16 == 8 for r in recs)


def _fresh(torch, F, g, n, like):
    return ([torch.empty_strided(like.shape, like.stride(), dtype=like.dtype, device="cuda") if like is not None else F.empty(n) for _ in g.ch.outs]
            + [torch.empty((n, F.nbytes), dtype=torch.uint8, device="cuda") for _ in g.ch.bouts] + [torch.empty(n, dtype=torch.int32, device="cuda") for _ in g.ch.pouts])


def test_outputs_in_the_arrays_of_inputs(ctx, torch_cuda, monkeypatch):
    """an element output in the array of an element input, an int output in the array of a selector, a byte output in the array of a byte
    input: a lane reads what it needs before it stores"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    ran = set()
    for g in progs:
        ch = g.ch
        ne, nb = len(ch.outs), len(ch.bouts)
        for path in _paths(g):
            _set(monkeypatch, path)
            n = _flat_n(g.ept)
            for kind, have in (("element", ch.nin and ne), ("int", ch.nsel and ch.pouts), ("byte", ch.bins and nb)):
                if not have:
                    continue
                mine = []

                def out(elems, recs, sels):
                    o = _fresh(torch, F, g, n, elems[0] if elems else None)
                    if kind == "element":
                        o[ne - 1] = elems[0]
                    elif kind == "int":
                        o[ne + nb] = sels[-1]
                    else:
                        o[ne] = recs[-1]
                    mine.append(o[{"element": ne - 1, "int": ne + nb, "byte": ne}[kind]])
                    return o
                _run(torch, F, g, g.f, n, (kind + " output on an input", path), width=n + 1, out=out, aliased=mine)
                ran.add(kind)
    assert {"element", "int"} <= ran and ("byte" in ran or not any(g.ch.bins for g in progs))


def test_element_major_entry(ctx, torch_cuda):
    """64 bits, programs without byte records (a chain with records has no such entry) that have an element input (the entry takes n
    from it): one chunk of 512 elements and 5 through f.aos()"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    if wl != 64:
        pytest.skip("the element-major entry is not built at word length 32")
    n, count = AOS_N, 0
    for g in progs:
        ch = g.ch
        if ch.bins or ch.bouts or not ch.nin:
            continue
        elems, _, sels = _inputs(torch, F, g, n)
        assert all(x.shape[1] == n for x in elems)
        aos = [F.to_aos(x) for x in elems]
        before = [t.clone() for t in aos + sels]
        got = g.f.aos(*aos, *g.shared, *sels)
        _compare(torch, F, g, [F.from_aos(x) for x in got[:len(ch.outs)]] + list(got[len(ch.outs):]), 0, n, "element-major")
        assert all(torch.equal(t, b) for t, b in zip(aos + sels, before))
        count += 1
    assert count >= 7                                            # (the light, heavy and long programs; 'unreduced' where the case has one)


def test_wider_builds_of_the_32_bit_form(ctx, torch_cuda, monkeypatch):
    """two and four elements per lane for the programs without a long exponentiation: the main launch at that width and the remainder"""
    torch = torch_cuda
    P, wl, F, progs = ctx
    if wl != 32:
        pytest.skip("64-bit chains are built at both of their widths: every test above runs them")
    count = 0
    for g in progs:
        for path in _paths(g):
            _set(monkeypatch, path)
            for e, f in g.wide.items():
                n = _flat_n(e)
                _, (elems, _, _) = _run(torch, F, g, f, n, ("ept = %d" % e, path), width=n + 1)
                assert all(x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0 for x in elems)
                _run(torch, F, g, f, 1, ("ept = %d, n = 1" % e, path))
                count += 1
    assert count >= 2 * 7


def test_unreduced_programs_agree_with_the_call_sequence(ctx):
    """docs/fused_chains.md: a chain with modshl or a negative modint takes no vote and runs the exact products, and the call-by-call
    sequence -- which votes per call -- leaves the same words.  The runs above held these programs to the oracle alone and noted where
    the call sequence differed; the documented claim is that it never does.  Runs last in the module"""
    P, wl, F, progs = ctx
    mine = [g for g in progs if g.profile == "unreduced"]
    if not mine:
        pytest.skip("the 'unreduced' profile is for X25519, NIST256 and X448 at 64 bits")
    for g in mine:
        assert g.runs >= 5 and not g.differs, (g.ch.name, g.differs)
