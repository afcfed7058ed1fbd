"""Seeded random programs for the chain compiler (tests/chain_programs.py), CPU side: the generator is deterministic and its seed set covers
what the compiler accepts; every program reads back from its text; the oracle interpreter and the integer model agree on every
64-bit program of the oracle's primes, which validates both before a GPU is involved; the test batch tells every program from its
single-operation mutants; every program cross-compiles for gfx950.  No compute on a GPU here."""
import os
import re
import sys

import pytest

from modarith_amd import _lib, fuse
from modarith_amd.fuse import parse
from tests import chain_programs as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64                                                           # the CPU batch: the 52 directed and seeded operands of the pool, then seeded ones


def _cases():
    return cp.available_cases()


@pytest.fixture(scope="module")
def built_lib():
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"


@pytest.fixture(scope="module", params=cp.CASES, ids=lambda c: "%s-w%d" % c)
def case(request, built_lib):
    P, wl = request.param
    if request.param not in _cases():
        pytest.skip("no plug-in of the generated field %s in this tree" % P)
    return P, wl, [cp.random_chain(P, wl, s, pr) for pr, s in cp.programs(P, wl)]


def _same_program(a, b):
    return (a.ops == b.ops and a.bins == b.bins and a.bouts == b.bouts and a.outs == b.outs and a.pouts == b.pouts and a.layout() == b.layout()
            and a.source() == b.source())


def test_a_seed_names_a_program(case):
    P, wl, chains = case
    again = [cp.random_chain(P, wl, s, pr) for pr, s in cp.programs(P, wl)]
    for a, b in zip(chains, again):
        assert _same_program(a, b) and a.text == b.text, a.name
    bodies = [cp.body_of(c) for c in chains]
    assert len(set(bodies)) == len(bodies)                      # different seeds, different programs
    assert not _same_program(cp.random_chain(P, wl, 1, "light"), cp.random_chain(P, wl, 2, "light"))
    for ch, (pr, s) in zip(chains, cp.programs(P, wl)):
        heavy = sum(o.op in fuse._HEAVY for o in ch.ops)
        assert heavy == 0 if pr != "heavy" else 1 <= heavy <= 3, ch.name
        assert len(ch.ops) == cp.LONG_OPS if pr == "long" else 8 <= len(ch.ops) <= 24, ch.name
        if pr == "bytes":
            assert ch.bins and ch.bouts
        if pr == "unreduced":                                    # no vote: the exact products throughout
            assert any(o.op == "modshl" or (o.op == "modint" and o.imm < 0) for o in ch.ops) and "bool fast = false;" in ch.source() and "&& false)" in ch.source()
        elif wl == 64 and P in cp.ORACLE_PRIMES:
            assert "&& true)" in ch.source(), ch.name            # ... and every other program of these fields takes it


def _ints_of(P, wl, data, oracle):
    if wl == 64 and P in cp.ORACLE_PRIMES:
        return lambda c: cp.run_oracle(c, oracle, *data)[2]
    return lambda c: cp.run_model(c, cp.fp_of(P, wl), *data)[2]  # (no oracle for this form: the model, where it is determined)


def test_the_seed_set_covers_what_the_compiler_accepts(case, oracle):
    """conditions, not measurements: tests/chain_programs.py required() lists them"""
    P, wl, chains = case
    got = set()
    for ch in chains:
        got |= cp.covered(ch, _ints_of(P, wl, cp.make_batch(ch, N), oracle))
    missing = cp.required(P, wl) - got
    assert not missing, sorted(missing, key=str)


def test_the_model_determines_three_quarters_of_the_outputs(case):
    P, wl, chains = case
    fp = cp.fp_of(P, wl)
    total = unknown = 0
    for ch in chains:
        E, B, I = cp.run_model(ch, fp, *cp.make_batch(ch, N))
        for col in E:
            total += len(col)
            unknown += sum(m.v is None and m.sq is None for m in col)
        for col in B + I:
            total += len(col)
            unknown += sum(x is None for x in col)
    assert 4 * unknown <= total, (unknown, total)


def test_text_round_trip(case):
    """every program has a text form: the language of fuse.parse lacks nothing the generator uses"""
    P, wl, chains = case
    without = [ch.name for ch in chains if ch.text is None]
    assert without == []
    for ch in chains:
        assert _same_program(parse(P, ch.name, ch.text, wl), ch), ch.name


@pytest.mark.parametrize("P", cp.ORACLE_PRIMES)
def test_oracle_interpreter_against_the_model(P, oracle, built_lib):
    """every determined output of the model is the value of the oracle's words, every determined int the oracle's int, every determined
    record the oracle's bytes: on the whole operand pool, for every 64-bit program"""
    fp = cp.fp_of(P, 64)
    checked = 0
    for pr, s in cp.programs(P, 64):
        ch = cp.random_chain(P, 64, s, pr)
        data = cp.make_batch(ch, N)
        E, B, I = cp.run_oracle(ch, oracle, *data)
        ME, MB, MI = cp.run_model(ch, fp, *data)
        free = cp.limb_free(ch)
        for k, (col, mcol) in enumerate(zip(E, ME)):
            for j, (row, m) in enumerate(zip(col, mcol)):
                ok = cp.model_agrees(fp, m, row, ch.outs[k] in free)
                assert ok is not False, (ch.name, "element output", k, "element", j)
                checked += ok is True
        for what, cols, mcols in (("byte", B, MB), ("int", I, MI)):
            for k, (col, mcol) in enumerate(zip(cols, mcols)):
                for j, (x, m) in enumerate(zip(col, mcol)):
                    assert m is None or m == x, (ch.name, what + " output", k, "element", j)
                    checked += m is not None
    assert checked > 5000


@pytest.mark.parametrize("P", cp.ORACLE_PRIMES)
def test_the_batch_tells_a_program_from_its_mutants(P, oracle, built_lib):
    """one live operation changed -- operands of modsub or modcmv swapped, the halves of modcsw swapped, another int as the selector,
    another shared operand, a record's byte order flipped -- and the oracle interpreter's outputs over the test batch differ: the
    comparison on the GPU would fail on an emitter that got one of these wrong"""
    classes = {"operands of modsub": 5, "operands of modcmv": 10, "dst and dst2 of modcsw": 10, "selector": 20, "shared operand": 8, "little flipped": 8}
    count = dict.fromkeys(classes, 0)
    for pr, s in cp.programs(P, 64):
        ch = cp.random_chain(P, 64, s, pr)
        data = cp.make_batch(ch, N)
        want = cp.run_oracle(ch, oracle, *data)
        for what, m in cp.mutants(ch):
            assert cp.run_oracle(m, oracle, *data) != want, (ch.name, what)
            kind, = [c for c in classes if c in what]
            count[kind] += 1
    for kind, least in classes.items():                          # no class of mutant has quietly gone from the seed set
        assert count[kind] >= least, (kind, count)


def _one_per_lane(ks):
    return [k for k in ks if re.search(r"<1[,>]", k["name"])]


def test_every_program_cross_compiles(case):
    """into chain_programs.plugin_dir(), where the GPU tests find them; every unit exports its _batch entry, and a program without a
    long exponentiation keeps every value in registers at one element per lane (docs/fused_chains.md says so of every such chain)"""
    P, wl, chains = case
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    built = cp.build_all(cp.available_cases(), workers=min(16, len(os.sched_getaffinity(0))))[(P, wl)]      # (every case the first time round)
    assert len(built) == len(cp.units(P, wl))
    for (pr, s, ept), f in built.items():
        ch = f.chain
        assert os.path.exists(f.path) and hasattr(f.lib, ch.symbol), ch.name
        assert hasattr(f.lib, "chain_%s_%s_aos" % (ch.name, P)) == (wl == 64)
        if ept is not None or ch._long():
            continue
        obj = f.path.replace("libmodarith_amd_chain_", "chain_")[:-3] + ".o"
        if not os.path.exists(obj):                              # (a plug-in that came without its object)
            f = ch.build(plugin_dir=cp.plugin_dir(), force=True)
        ks = kernel_resources.kernels_of(obj)
        one = _one_per_lane(ks)
        assert one, [k["name"] for k in ks]
        for k in one:
            assert k["private_segment_fixed_size"] == 0, (ch.name, k)     # (registers spilled into accumulation registers are recorded, not asserted)


def test_the_recorded_resources_name_the_units_of_the_seed_set(case):
    """profiles/chain_programs_resources.json is written by `python -m tests.chain_programs --resources`; its figures are recorded, not
    asserted, but it is the record of THIS seed set: a unit for every (program, case, width), and kernels under each"""
    import json
    P, wl, _ = case
    rec = json.load(open(os.path.join(ROOT, cp.RESOURCES)))["programs"]
    for pr, s, ept in cp.units(P, wl):
        assert rec.get(cp.resource_key(pr, s, P, wl, ept)), (pr, s, ept)
    mine = [k for k in rec if "/%s/w%d" % (P, wl) in k]
    assert len(mine) == len(cp.units(P, wl))


def test_what_the_builder_accepts_of_generic_false_results(oracle, built_lib):
    """Found by the random programs, pinned here as it stands.  The builder refuses a generic=False operation on a generic=False result
    and says `reduce in between (modadd / modsub / modmul ...)`; it takes modneg for such a reduction, and it does not follow a lazy
    value through modcpy / modcmv / modcsw.  modadd_lazy(modneg(modsub_lazy(a, b)), c) is accepted, and on the oracle -- field.c itself --
    it leaves elements whose top limb is below zero: values right mod p, limbs outside what redc, the predicates and modexp are for.
    The generator therefore feeds generic=False results to products only (docs/fused_chains.md, "Random programs": a limit of what the
    seed set covers).  Whether the builder should refuse these is not decided here"""
    from modarith_amd.fuse import Chain
    ch = Chain("X25519", "neglazy")
    a, b, c = ch.inputs(3)
    with pytest.raises(ValueError, match="reduce in between"):
        ch.modadd_lazy(ch.modsub_lazy(a, b), c)
    ch = Chain("X25519", "neglazy")
    a, b, c = ch.inputs(3)
    ch.output(ch.modadd_lazy(ch.modneg(ch.modsub_lazy(a, b)), c))            # accepted
    ch.output(ch.modneg_lazy(ch.modcpy(ch.modsub_lazy(a, b))))               # accepted: a copy of a lazy value is not tracked
    ch.notes = {"progenitor_of": {}}
    data = cp.make_batch(ch, N)
    E, _, _ = cp.run_oracle(ch, oracle, *data)
    fp = cp.fp_of("X25519", 64)
    negative = [j for j, row in enumerate(E[0]) if row[-1] >> 63]
    assert negative, "the oracle no longer leaves a negative element here: the generator's rule can go"
    M, _, _ = cp.run_model(ch, fp, *data)
    assert all(cp.model_agrees(fp, m, row) for m, row in zip(M[0], E[0]))     # (right mod p, the top limb read as a signed word)
