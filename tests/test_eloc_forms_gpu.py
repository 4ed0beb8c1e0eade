"""The local-energy path of naqs_hip.hip at every kernel instance its dispatcher can form, against the CPU oracle: what
tests/test_forward_f64_gpu.py is for the log-psi forward and tests/test_backward_gpu.py for the training backward.

Inputs come from tests/test_eloc_forms.py, which proves without a GPU that they are what they claim: Hamiltonians with groups of
8, 9, 17, 64, 65, 255, 256 and 300 terms (the edges of eloc_kernel's heavy path and of eloc_kernel2's chunked view) at 32- and
64-bit keys, with and without the sector filter, bit N-1 in play; and 512-key tables whose keys all hash to the key table's
last slot, so that every look-up walks a chain that wraps the table's end — a hit deep inside it, a miss all 512 taken slots
to the first free one.  Every instance NAME is asserted (`naqs_ham_last_kernel`) against the mirrors of the dispatcher in that
module, so that an instance which silently stops being reachable fails here.

Bounds: 1e-10 relative against the oracle (tests/test_eloc_gpu.py's), 1e-12 between the two kernel versions (its
test_single_and_double_compaction_kernels_agree), bit equality across STAGE, NT, the filter, rows per block and row shards of
one kernel version, and for the weighted sums n 2^-53 sum |terms| against the exactly rounded sum.

Wall time of the module on an MI355X: 35 tests in 5.7 s, 3.6 s of it inside the tests (profiles/eloc_forms.txt).
"""
import contextlib
import os
import time
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

import test_eloc_forms as F
from test_eloc_gpu import env, rel_err, run_eloc, synth_logpsi  # noqa: F401 (env: fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KINDS = {"f32": (32, 8, 8, True), "u32": (32, 8, 8, False), "f64": (40, 6, 6, True), "u64": (40, 6, 6, False)}
WIDTHS = {32: (32, 8, 8), 64: (40, 6, 6)}
SMALL_ROWS = 37
REPORT = {kb: dict(worst=0.0, worst_case="", names=set(), calls=0) for kb in (32, 64)}
T0 = time.time()


@contextlib.contextmanager
def naqs_env(**kw):
    """Set NAQS_<NAME> for the block (None: leave unset) and put back what was there."""
    names = {f"NAQS_{k}": v for k, v in kw.items()}
    old = {k: os.environ.get(k) for k in names}
    try:
        for k, v in names.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _report():
    """NAQS_ELOC_FORMS_REPORT=<file>: what the module saw, for profiles/eloc_forms.txt."""
    yield
    path = os.environ.get("NAQS_ELOC_FORMS_REPORT")
    if not path:
        return
    with open(path, "w") as f:
        for kb in (32, 64):
            r = REPORT[kb]
            packed, a, b = F.crowded(kb)
            look = F.lookups(packed, a, kb, pool=np.r_[a, b])
            f.write(f"uint{kb}_t: {r['calls']} calls checked against the oracle, worst rel_err {r['worst']:.3e} ({r['worst_case']})\n")
            f.write(f"uint{kb}_t: longest chain walked by one look-up: {look['longest']} slots (512-key crowded table: "
                    f"{look['hits']} hits on {look['rows_hit']} rows, {look['absent_pool']} misses through the whole chain)\n")
            f.write(f"uint{kb}_t: {len(r['names'])} instance names seen\n")
            for n in sorted(r["names"]):
                f.write(f"    {n}\n")
        f.write(f"module wall time {time.time() - T0:.1f} s\n")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def wave_function(M, seed):
    lp = synth_logpsi(M, seed)
    psi = np.exp(lp[:, 0] + 1j * lp[:, 1])
    return psi, np.stack([psi.real, psi.imag], -1)


def oracle(env, packed, keys, psi):
    return env["O"].eloc_matrix_free(packed.xy, packed.yz, packed.coeff, keys, psi)


def eloc(env, ham, keys, wf, **kw):
    return run_eloc(env, ham, keys, wf, dtype=torch.float64, **kw)


def held(kb, e, want, case):
    """The oracle bound of every call of this module; the worst figure is kept for the report."""
    err = float(rel_err(e, want))
    r = REPORT[kb]
    r["calls"] += 1
    if err > r["worst"]:
        r["worst"], r["worst_case"] = err, str(case)
    assert err < 1e-10, (case, err)


def named(kb, ham, want_name):
    got = ham.last_kernel()
    REPORT[kb]["names"].add(got)
    assert got == want_name
    return got


def expected_name(packed, n_rows, v2=True, block=None, stage=2, filter_built=False):
    """The instance `launch_main` picks: NT from NAQS_BLOCK or the row count, the filter only at 1024 threads, the STAGE the
    smaller of the forced one and what fits the LDS."""
    kb = 32 if packed.n_qubits <= 32 else 64
    nt = block or F.default_block(n_rows)
    bloom = bool(filter_built) and nt == 1024
    return F.kernel_name(kb, v2, min(stage, F.natural_stage(packed, nt, v2, bloom)), nt, bloom)


# ------------------------------------------------------------------------------------------- cases, built once
@lru_cache(maxsize=None)
def heavy_case(kind):
    N, na, nb, filtered = KINDS[kind]
    keys = F.matrix_keys(N, na, nb)
    packed = F.ham_with_heavy_groups(keys, F.MATRIX_MASKS, 5, na if filtered else -1, nb if filtered else -1, N)
    psi, wf = wave_function(len(keys), 3)
    return packed, keys, psi, wf


_WANT = {}


def heavy_want(env, kind, M):
    if (kind, M) not in _WANT:
        packed, keys, psi, _ = heavy_case(kind)
        _WANT[kind, M] = oracle(env, packed, keys[:M], psi[:M])
    return _WANT[kind, M]


@lru_cache(maxsize=None)
def big_case(kb):
    """A pool of BLOOM_MIN_ROWS + 1 keys of the width's sector in random order and a light Hamiltonian of ~900 terms over it,
    whose leading masks join the pool's first keys (a short prefix of the pool is a table that still couples)."""
    N, na, nb = WIDTHS[kb]
    keys = F._pool(N, na, nb, F.BLOOM_MIN_ROWS + 1, 31).copy()
    packed = F.ham_light(keys, 300, 37, na, nb, N)
    psi, wf = wave_function(len(keys), 41)
    return packed, keys, psi, wf


def big_want(env, kb, M):
    if ("big", kb, M) not in _WANT:
        packed, keys, psi, _ = big_case(kb)
        _WANT["big", kb, M] = oracle(env, packed, keys[:M], psi[:M])
    return _WANT["big", kb, M]


# ------------------------------------------------------------------------------------------- the instance matrix
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_instance_against_the_oracle(env, kind):
    """{eloc_kernel2, eloc_kernel} x NT {256, 512, 1024, default} x STAGE {2, 1, 0} x filter {off, on} at three row counts: the
    name is the requested instance, E_loc is within 1e-10 of the oracle, one kernel version gives ONE set of bits whatever the
    shape, the two versions agree to 1e-12, and the names seen are every instance the dispatcher can form at this key width."""
    packed, keys, psi, wf = heavy_case(kind)
    kb = 32 if packed.n_qubits <= 32 else 64
    ham = env["H"].DevicePauliHamiltonian(packed)
    assert ham.key_bits == kb
    seen, first = set(), {}
    for v in (2, 1):
        for block in (None, 256, 512, 1024):
            nwaves = (block or F.default_block(1)) // F.WAVE
            for M in (SMALL_ROWS, F.MATRIX_ROWS, nwaves + 1):
                want = heavy_want(env, kind, M)
                for stage in (2, 1, 0):
                    for bloom in (0, 1):
                        with naqs_env(ELOC_V=v if v == 1 else None, BLOCK=block, STAGE=stage, BLOOM=bloom):
                            e = eloc(env, ham, keys[:M], wf[:M])
                        case = (kind, v, block, M, stage, bloom)
                        seen.add(named(kb, ham, expected_name(packed, M, v == 2, block, stage, bloom)))
                        held(kb, e, want, case)
                        assert np.array_equal(e, first.setdefault((v, M), e)), case
    for (v, M), e in first.items():
        if v == 1:
            assert rel_err(e, first[2, M]) < 1e-12, M
    assert seen == F.all_kernel_names(kb), sorted(F.all_kernel_names(kb) - seen)
    assert np.count_nonzero(np.abs(heavy_want(env, kind, F.MATRIX_ROWS).imag) > 1e-9) > F.MATRIX_ROWS // 20     # rows couple


@pytest.mark.parametrize("kind", list(KINDS))
def test_rows_per_block_and_shards_keep_the_bits(env, kind):
    packed, keys, psi, wf = heavy_case(kind)
    kb = 32 if packed.n_qubits <= 32 else 64
    ham = env["H"].DevicePauliHamiltonian(packed)
    M = F.MATRIX_ROWS
    rs = np.random.RandomState(7)
    for v in (2, 1):
        with naqs_env(ELOC_V=v if v == 1 else None):
            full = eloc(env, ham, keys, wf)
            held(kb, full, heavy_want(env, kind, M), (kind, v, "full"))
            for rpb in (1, 3, F.default_block(M) // F.WAVE, 1000):
                with naqs_env(ROWS_PER_BLOCK=rpb):
                    assert np.array_equal(eloc(env, ham, keys, wf), full), (v, rpb)
            # shards: fixed cuts around the block-shape switch and random ones; a shard below BIG_BLOCK_ROWS runs NT = 512
            for cuts in ([0, 1, F.BIG_BLOCK_ROWS, M], [0, M - F.BIG_BLOCK_ROWS, M], np.r_[0, np.sort(rs.choice(M, 4, replace=False)), M]):
                parts = []
                for b, e_ in zip(cuts[:-1], cuts[1:]):
                    parts.append(eloc(env, ham, keys, wf, row_begin=int(b), n_rows=int(e_ - b)))
                    if e_ > b:
                        named(kb, ham, expected_name(packed, int(e_ - b), v == 2))
                assert np.array_equal(np.concatenate(parts), full), (v, list(cuts))


CHUNK_KINDS = dict(KINDS, s32=(20, 5, 5, True))          # a sector below 2^20 states: the short chunk is its default


@lru_cache(maxsize=None)
def chunk_case(kind):
    if kind in KINDS:
        return heavy_case(kind)
    N, na, nb, _ = CHUNK_KINDS[kind]
    keys = F._pool(N, na, nb, F.MATRIX_ROWS, 17).copy()
    psi, wf = wave_function(len(keys), 3)
    return F.ham_with_heavy_groups(keys, F.MATRIX_MASKS, 5, na, nb, N), keys, psi, wf


@pytest.mark.parametrize("kind", list(CHUNK_KINDS))
def test_chunk_lengths(env, kind):
    """eloc_kernel2's view at chunk lengths 1, 8, 9, 64 and 255 (NAQS_CHUNK_TERMS, read when the handle is made): each within
    1e-10 of the oracle, and the default handle's bits are those of the length its sector selects."""
    packed, keys, psi, wf = chunk_case(kind)
    kb = 32 if packed.n_qubits <= 32 else 64
    want = oracle(env, packed, keys, psi)
    res = {}
    for c in (None, 1, 8, 9, 64, 255):
        with naqs_env(CHUNK_TERMS=c):
            ham = env["H"].DevicePauliHamiltonian(packed)
        res[c] = eloc(env, ham, keys, wf)
        named(kb, ham, F.kernel_name(kb, True, F.natural_stage(packed, 1024, True, chunk=c), 1024, 0))
        held(kb, res[c], want, (kind, "chunk", c))
    own = F.chunk_terms(packed.n_qubits, packed.n_alpha, packed.n_beta)
    assert own == (F.HEAVY_TERMS if kind == "s32" else F.LONG_CHUNK)
    assert np.array_equal(res[None], res[own])


def test_stage_0_and_1_unforced(env):
    """64-bit Hamiltonians whose size alone selects STAGE 0 (the group view is beyond the LDS budget) and STAGE 1."""
    keys = F._pool(40, 6, 6, 2000, 19).copy()
    psi, wf = wave_function(len(keys), 13)
    for stage, packed in zip((0, 1), F.stage_hams(keys)):
        ham = env["H"].DevicePauliHamiltonian(packed)
        want = oracle(env, packed, keys, psi)
        for v in (2, 1):
            with naqs_env(ELOC_V=v if v == 1 else None):
                e = eloc(env, ham, keys, wf)
            named(64, ham, F.kernel_name(64, v == 2, stage, 1024, 0))
            held(64, e, want, ("natural stage", stage, v))


# ------------------------------------------------------------------------------------------- table sizes
def size_classes():
    """Row counts at which the dispatch changes, from the source's constants and the device: 1; nwaves - 1, nwaves, nwaves + 1
    of each block shape; the switch to 1024 threads; 32 CUs, where rows_per_block leaves nwaves; the filter's default."""
    rows = {1}
    for pivot in (*F.NWAVES, F.BIG_BLOCK_ROWS, 32 * cus(), F.BLOOM_MIN_ROWS):
        rows |= {pivot - 1, pivot, pivot + 1}
    return sorted(r for r in rows if r >= 1)


@pytest.mark.parametrize("kb", [32, 64])
def test_size_classes(env, kb):
    packed, keys, psi, wf = big_case(kb)
    ham = env["H"].DevicePauliHamiltonian(packed)
    rows = size_classes()
    assert rows[-1] == len(keys) and len(rows) >= 18
    for M in rows:
        e = eloc(env, ham, keys[:M], wf[:M])
        named(kb, ham, expected_name(packed, M, filter_built=M >= F.BLOOM_MIN_ROWS))
        held(kb, e, big_want(env, kb, M), ("size", M))
    assert np.count_nonzero(np.abs(big_want(env, kb, len(keys)).imag) > 1e-9) > 200


@pytest.mark.parametrize("kb", [32, 64])
def test_filter_built_and_not_used(env, kb):
    """prep_kernel fills the filter for the whole table; a row shard below 1024 rows, or a forced filter at 512 threads, runs
    an instance that never reads it.  Same bits as the rows of the call that does."""
    packed, keys, psi, wf = big_case(kb)
    ham = env["H"].DevicePauliHamiltonian(packed)
    M = len(keys)
    full = eloc(env, ham, keys, wf)
    named(kb, ham, expected_name(packed, M, filter_built=True))
    assert "BLOOM=1" in ham.last_kernel()
    held(kb, full, big_want(env, kb, M), ("filter", M))
    part = eloc(env, ham, keys, wf, row_begin=5, n_rows=100)
    assert "NT=512, BLOOM=0" in named(kb, ham, expected_name(packed, 100, filter_built=True))
    assert np.array_equal(part, full[5:105])
    part = eloc(env, ham, keys, wf, row_begin=7, n_rows=F.BIG_BLOCK_ROWS + 1)
    assert "NT=1024, BLOOM=1" in named(kb, ham, expected_name(packed, F.BIG_BLOCK_ROWS + 1, filter_built=True))
    assert np.array_equal(part, full[7:7 + F.BIG_BLOCK_ROWS + 1])
    m = 700
    with naqs_env(BLOOM=1):
        on = eloc(env, ham, keys[:m], wf[:m])
        assert "NT=512, BLOOM=0" in named(kb, ham, expected_name(packed, m, filter_built=True))
    with naqs_env(BLOOM=0):
        off = eloc(env, ham, keys[:m], wf[:m])
    held(kb, on, big_want(env, kb, m), ("filter", m))
    assert np.array_equal(on, off)


# ------------------------------------------------------------------------------------------- the crowded key table
@lru_cache(maxsize=None)
def crowded_tables(kb):
    packed, a, b = F.crowded(kb)
    sub = np.random.RandomState(5).choice(len(a), 37, replace=False)
    tabs = {}
    for name, keys, seed in (("A", a, 51), ("B", b, 52), ("A37", a[sub], 53)):
        psi, wf = wave_function(len(keys), seed)
        tabs[name] = (keys, psi, wf)
    return packed, tabs


def crowded_want(env, kb, name):
    if ("crowded", kb, name) not in _WANT:
        packed, tabs = crowded_tables(kb)
        keys, psi, _ = tabs[name]
        _WANT["crowded", kb, name] = oracle(env, packed, keys, psi)
    return _WANT["crowded", kb, name]


@pytest.mark.parametrize("kb", [32, 64])
def test_crowded_table_every_family(env, kb):
    """512 keys on ONE home slot, the table's last: every hit is found down a chain that wraps the table's end, every miss
    among the pool's other half walks all 512 taken slots.  Both kernels x STAGE {2, 1, 0} at the default block shape and at
    1024 threads with the filter."""
    packed, tabs = crowded_tables(kb)
    keys, psi, wf = tabs["A"]
    want = crowded_want(env, kb, "A")
    assert np.count_nonzero(np.abs(want.imag) > 1e-9) >= 0.4 * len(keys)
    ham = env["H"].DevicePauliHamiltonian(packed)
    first = {}
    for v in (2, 1):
        for block, bloom in ((None, 0), (1024, 1)):
            for stage in (2, 1, 0):
                with naqs_env(ELOC_V=v if v == 1 else None, BLOCK=block, STAGE=stage, BLOOM=bloom):
                    e = eloc(env, ham, keys, wf)
                named(kb, ham, expected_name(packed, len(keys), v == 2, block, stage, bloom))
                held(kb, e, want, ("crowded", v, block, stage, bloom))
                assert np.array_equal(e, first.setdefault(v, e)), (v, block, stage)
    assert rel_err(first[1], first[2]) < 1e-12


@pytest.mark.parametrize("kb", [32, 64])
def test_crowded_table_stale_epochs_and_the_epoch_wrap(env, kb):
    """One handle: table A, table B (the pool's other half, the same home slot), 37 keys of A, A again — the slots of each call
    lie as stale entries under the next one's chain — then 260 alternating calls, which take the 8-bit epoch through its wrap
    with the chain in place, and both tables once more."""
    packed, tabs = crowded_tables(kb)
    ham = env["H"].DevicePauliHamiltonian(packed)
    for name in ("A", "B", "A37", "A"):
        keys, psi, wf = tabs[name]
        held(kb, eloc(env, ham, keys, wf), crowded_want(env, kb, name), ("stale", name))
    dev = {n: (env["H"].keys_to_device(tabs[n][0], ham.device), torch.as_tensor(tabs[n][2], device=ham.device)) for n in "AB"}
    for it in range(260):
        ham.local_energy(*dev["AB"[it % 2]])
    torch.cuda.synchronize()
    for name in ("A", "B"):
        keys, psi, wf = tabs[name]
        held(kb, eloc(env, ham, keys, wf), crowded_want(env, kb, name), ("after the wrap", name))


# ------------------------------------------------------------------------------------------- naqs_hmatvec
@pytest.mark.parametrize("kind", ["f32", "u64"])
def test_hmatvec_through_the_same_instances(env, kind):
    """(H v)_i = conj(E_loc_i) v_i with the oracle's E_loc for psi = v: both key widths x STAGE {2, 0} x NT {512, 1024}, a
    complex and a real v, on rows where |v_i| is not small (the oracle divides by it)."""
    packed, keys, _, _ = heavy_case(kind)
    kb = 32 if packed.n_qubits <= 32 else 64
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = env["H"].keys_to_device(keys, ham.device)
    rs = np.random.RandomState(61)
    M = len(keys)
    for v in (rs.normal(size=M) + 1j * rs.normal(size=M), rs.normal(size=M) + 0j):
        want = np.conj(oracle(env, packed, keys, v)) * v
        rows = np.abs(v) > 0.05
        assert rows.sum() > 0.9 * M
        vt = torch.as_tensor(v.real.copy() if not v.imag.any() else np.stack([v.real, v.imag], -1), device=ham.device)
        for stage in (2, 0):
            for block in (512, 1024):
                with naqs_env(STAGE=stage, BLOCK=block):
                    got = ham.matvec(kd, vt)
                    torch.cuda.synchronize()
                named(kb, ham, expected_name(packed, M, True, block, stage))
                got = got.cpu().numpy()
                got = got if got.ndim == 1 else got[:, 0] + 1j * got[:, 1]
                err = np.max(np.abs(got - want)[rows] / np.maximum(1.0, np.abs(want))[rows])
                assert err < 1e-10, (kind, stage, block, err)


# ------------------------------------------------------------------------------------------- reduce_kernel
REDUCE_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 20001)


def _exact_sums(w, e):
    """The four weighted sums and the sums of their terms' magnitudes, exactly (rational arithmetic on the doubles)."""
    W = [Fraction(float(x)) for x in w]
    R = [Fraction(float(x)) for x in e[:, 0]]
    Im = [Fraction(float(x)) for x in e[:, 1]]
    terms = ([a * r for a, r in zip(W, R)], [a * i for a, i in zip(W, Im)], [a * r * r for a, r in zip(W, R)], W)
    return [sum(t, Fraction(0)) for t in terms], [sum((abs(x) for x in t), Fraction(0)) for t in terms]


@pytest.mark.parametrize("n", REDUCE_SIZES)
def test_reduce_kernel_sizes(env, n):
    """naqs_eloc_reduce at sizes around a wave, the workgroup and its eight-element batches: integer weights from 1 to 10^12,
    E_loc = -107 +- 1e-3, so that sum w Re^2 is huge next to the variance it is there for.  Each sum within n 2^-53 sum |terms|
    of the exact one: (n - 1) 2^-53 is the a-priori bound of ANY summation order, one more rounding for the product (w Re^2 is
    two rounded products in a build without contraction and is held to the same figure; profiles/eloc_forms.txt).  Then
    naqs_eloc_reduced == naqs_eloc followed by naqs_eloc_reduce, bit for bit, on a table of n rows."""
    packed, keys, psi, wf = big_case(32)
    ham = env["H"].DevicePauliHamiltonian(packed)
    rs = np.random.RandomState(1000 + n)
    w = np.floor(10.0 ** rs.uniform(0, 12, n))
    if n >= 2:
        w[0], w[1 + rs.randint(n - 1)] = 1.0, 1e12
    e = np.stack([-107.0 + 1e-3 * rs.normal(size=n), 1e-3 * rs.normal(size=n)], -1)
    got = ham.reduce(torch.as_tensor(w, device=ham.device), torch.as_tensor(e, device=ham.device)).cpu().numpy()
    exact, mags = _exact_sums(w, e)
    for k in range(4):
        err, bound = abs(Fraction(float(got[k])) - exact[k]), n * Fraction(1, 2 ** 53) * mags[k]
        print(f"n={n} sum {k}: error {float(err):.3e}, bound {float(bound):.3e}")
        assert err <= bound, (n, k, float(err), float(bound))
    kd = env["H"].keys_to_device(keys[:n], ham.device)
    wd, wfd = torch.as_tensor(w, device=ham.device), torch.as_tensor(wf[:n], device=ham.device)
    e1, s1 = ham.local_energy(kd, wfd, weights=wd)
    e2 = ham.local_energy(kd, wfd)
    s2 = ham.reduce(wd, e2)
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and torch.equal(s1, s2)
