"""eloc_kernel2's closed forms (class D sign tables, class S segment tables) on the GPU: against the term
loop of the same build (NAQS_ELOC_CLOSED=0, read when the handle is created), against the single-compaction kernel
(NAQS_ELOC_V=1) and against the CPU oracle.

Bounds: 1e-12 (`rel_err` of test_eloc_gpu.py) between the forms of one build — the bound the two kernel versions already
hold to each other; 1e-10 against the oracle; bitwise where only the launch differs, and for Hamiltonians whose groups are
all class D (a D table entry is the loop's own sum)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import closed_reference as cr
from conftest import GOLDEN, golden
from test_eloc_gpu import all_keys, random_physical_keys, rel_err, synth_logpsi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def env():
    from naqs_amd import _lib, hamiltonian, packing
    from oracle import oracle
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load_library()
    return dict(lib=_lib, H=hamiltonian, P=packing, O=oracle)


def handle(env, packed, closed=True, **create_env):
    """A handle whose view is built with the closed forms on or off (the switch is read at creation and kept)."""
    with environ(NAQS_ELOC_CLOSED=1 if closed else 0, **create_env):
        return env["H"].DevicePauliHamiltonian(packed)


def run(env, ham, keys, psi, **kw):
    k = env["H"].keys_to_device(np.asarray(keys, np.uint64), ham.device)
    w = torch.as_tensor(np.stack([psi.real, psi.imag], -1), dtype=torch.float64, device=ham.device)
    e = ham.local_energy(k, w, kind="psi", **kw)
    torch.cuda.synchronize()
    e = e.cpu().numpy()
    return e[:, 0] + 1j * e[:, 1]


def synth_psi(M, seed):
    lp = synth_logpsi(M, seed)
    return np.exp(lp[:, 0] + 1j * lp[:, 1])


def packed_of(env, mol, filtered=True, keep=None):
    h = golden(f"ham_{mol}.npz")
    xy, yz, cf = h["xy"], h["yz"], h["coeff"]
    if keep is not None:
        m = keep(xy)
        xy, yz, cf = xy[m], yz[m], cf[m]
    na, nb = (int(h["n_alpha"]), int(h["n_beta"])) if filtered else (-1, -1)
    return env["P"].PackedHamiltonian(int(h["n_qubits"]), na, nb, xy, yz, cf)


def chunk_terms(packed):
    from test_eloc_forms import chunk_terms as mirror
    return mirror(packed.n_qubits, packed.n_alpha, packed.n_beta)


# ------------------------------------------------------------------ golden Hamiltonians
_CASES = {}


def golden_case(env, mol):
    """Keys, psi and the oracle's E_loc at the three table sizes, computed once per molecule."""
    if mol not in _CASES:
        h = golden(f"ham_{mol}.npz")
        space = all_keys(int(h["n_qubits"]), int(h["n_alpha"]), int(h["n_beta"]))
        rs = np.random.RandomState(31)
        out = {}
        for M in (1, 512 // 64 + 1, 300):                    # one row; one more than a 512-thread workgroup's waves; 300
            keys = rs.permutation(rs.choice(space, min(M, len(space)), replace=False))
            psi = synth_psi(len(keys), 7 + M)
            out[M] = (keys, psi, env["O"].eloc_matrix_free(h["xy"], h["yz"], h["coeff"], keys, psi))
        _CASES[mol] = out
    return _CASES[mol]


@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("mol", ["LiH", "H2O", "N2"])
def test_golden_closed_against_loop_and_oracle(env, mol, filtered):
    packed = packed_of(env, mol, filtered)
    closed, loop = handle(env, packed, True), handle(env, packed, False)
    want_counts = cr.handle_counts(packed.xy, packed.yz, packed.coeff, packed.n_qubits, chunk_terms(packed))
    assert closed.closed_counts() == want_counts and want_counts[2] == 0 and want_counts[0] > 0 and want_counts[1] > 0
    n_groups = sum(want_counts[:3])
    assert loop.closed_counts() == (0, 0, n_groups, 0)
    for M, (keys, psi, want) in golden_case(env, mol).items():
        e_c, e_l = run(env, closed, keys, psi), run(env, loop, keys, psi)
        assert "eloc_kernel2<" in closed.last_kernel() and "eloc_kernel2<" in loop.last_kernel()
        with environ(NAQS_ELOC_V=1):
            e_1 = run(env, closed, keys, psi)
            assert "eloc_kernel<" in closed.last_kernel()
        print(f"{mol} filtered={filtered} M={len(keys)}: closed-loop {rel_err(e_c, e_l):.2e} closed-v1 {rel_err(e_c, e_1):.2e} "
              f"closed-oracle {rel_err(e_c, want):.2e}")
        assert rel_err(e_c, e_l) <= 1e-12 and rel_err(e_c, e_1) <= 1e-12
        assert rel_err(e_c, want) <= 1e-10 and rel_err(e_l, want) <= 1e-10


@pytest.mark.parametrize("mol", ["LiH", "H2O", "N2"])
def test_diagonal_and_doubles_only_are_bitwise_the_loop(env, mol):
    packed = packed_of(env, mol, keep=lambda xy: np.array([bin(int(x)).count("1") in (0, 4) for x in xy]))
    closed, loop = handle(env, packed, True), handle(env, packed, False)
    nd, ns, nl, _ = closed.closed_counts()
    assert nd == len(np.unique(packed.xy)) - 1 and ns == nl == 0
    keys, psi, _ = golden_case(env, mol)[300]
    e_c, e_l = run(env, closed, keys, psi), run(env, loop, keys, psi)
    assert np.count_nonzero(e_c) == len(keys) and np.array_equal(e_c, e_l)


# ------------------------------------------------------------------ synthetic Hamiltonians
def _deposit(mask, rs):
    """A random subset of the mask's bits."""
    return sum(1 << q for q in range(64) if (mask >> q) & 1 and rs.randint(2))


def _rand_bits(rs, N):
    return int(rs.randint(0, 1 << 30)) | (int(rs.randint(0, 1 << 30)) << 30) & ((1 << N) - 1) if N > 30 else int(rs.randint(0, 1 << N))


def d_terms(rs, xy, N, n=None):
    R = _rand_bits(rs, N) & ((1 << N) - 1)
    subs = {_deposit(xy, rs) for _ in range(n or rs.randint(1, 9))}
    return [R ^ s for s in sorted(subs)]


def s_terms(rs, xy, N, n=None):
    R = _rand_bits(rs, N) & ((1 << N) - 1)
    free = [q for q in range(N) if not (xy >> q) & 1]
    spect = [free[0], free[-1]] + [free[rs.randint(len(free))] for _ in range((n or rs.randint(5, 40)) - 3)]
    # (the first term has no spectator: the class needs a reference among the group's OWN terms)
    return [R ^ _deposit(xy, rs)] + [R ^ _deposit(xy, rs) ^ (0 if rs.rand() < 0.15 else 1 << q) for q in spect]


def excitation(rs, key, N, spin):
    occ = [q for q in range(spin, N, 2) if (key >> q) & 1]
    emp = [q for q in range(spin, N, 2) if not (key >> q) & 1]
    return (1 << occ[rs.randint(len(occ))]) | (1 << emp[rs.randint(len(emp))])


def synthetic(env, N, na, nb, seed, n_keys=500, fallbacks=False, filtered=True):
    """A cluster of physical keys grown by single and double excitations, and a Hamiltonian over exactly those flips: the
    diagonal, class-D groups (<= 8 terms inside the flipped bits), class-S groups (5-39 terms, spectators from bit 0 to bit
    N - 1), one mask of each kind flipping bit N - 1; with `fallbacks` also groups that must stay in the loop."""
    rs = np.random.RandomState(seed)
    base = int(random_physical_keys(N, na, nb, 1, seed)[0])
    top = 1 << (N - 1)
    keys, masks = [base], []

    def connect(k, m):
        if m not in masks:
            masks.append(m)
        if k ^ m not in keys:
            keys.append(k ^ m)

    # bit N - 1 (a beta orbital for even N) in a single and in a double
    beta = [q for q in range(1, N - 1, 2) if ((base >> q) & 1) != ((base >> (N - 1)) & 1)]
    connect(base, top | (1 << beta[0]))
    connect(base, top | (1 << beta[-1]) | excitation(rs, base, N, 0))
    six = []
    while len(keys) < n_keys:
        k = keys[rs.randint(len(keys))]
        m = excitation(rs, k, N, rs.randint(2))
        if rs.rand() < 0.6:
            m ^= excitation(rs, k ^ m, N, rs.randint(2))
        if fallbacks and rs.rand() < 0.05:
            m ^= excitation(rs, k ^ m, N, 0) ^ excitation(rs, k ^ m, N, 1)
        pc = bin(m).count("1")
        if pc in (2, 4) or (pc == 6 and fallbacks):
            connect(k, m)
            if pc == 6:
                six.append(m)
    xy, yz = [0] * 30, [_rand_bits(rs, N) & ((1 << N) - 1) for _ in range(30)]
    kinds = {}
    for i, m in enumerate(masks):
        pc = bin(m).count("1")
        if pc == 4:
            t = d_terms(rs, m, N)
            kinds[m] = "D"
            if fallbacks and i % 7 == 3:                    # one term carries a spectator bit
                free = [q for q in range(N) if not (m >> q) & 1]
                t.append(t[0] ^ (1 << free[rs.randint(len(free))]))
                kinds[m] = "L"
        elif pc == 2:
            t = s_terms(rs, m, N)
            kinds[m] = "S"
            if fallbacks and i % 5 == 2:                    # a term two spectators away from every other
                free = [q for q in range(N) if not (m >> q) & 1]
                t = [t[0], t[0] ^ (1 << free[1]) ^ (1 << free[2]) ^ (1 << free[3]), t[0] ^ (1 << free[4])]
                kinds[m] = "L"
        else:
            t = d_terms(rs, m, N, 5)
            kinds[m] = "L"
        xy += [m] * len(t)
        yz += t
    xy, yz = np.array(xy, np.uint64), np.array(yz, np.uint64)
    cf = rs.normal(size=len(xy))
    perm = rs.permutation(len(xy))
    packed = env["P"].PackedHamiltonian(N, na if filtered else -1, nb if filtered else -1, xy[perm], yz[perm], cf[perm])
    keys = rs.permutation(np.array(keys, np.uint64))
    assert np.any(keys & np.uint64(top)) and np.any(xy & np.uint64(top)) and np.any(yz & np.uint64(top))
    return packed, keys, kinds


def check_synthetic(env, packed, keys, counts, **create_env):
    closed, loop = handle(env, packed, True, **create_env), handle(env, packed, False)
    assert closed.closed_counts()[:3] == counts[:3], (closed.closed_counts(), counts)
    assert closed.closed_counts() == counts
    psi = synth_psi(len(keys), 3)
    want = env["O"].eloc_matrix_free(packed.xy, packed.yz, packed.coeff, keys, psi)
    e_c, e_l = run(env, closed, keys, psi), run(env, loop, keys, psi)
    name = closed.last_kernel()
    with environ(NAQS_ELOC_V=1):
        e_1 = run(env, closed, keys, psi)
    print(f"N={packed.n_qubits} counts {counts}: closed-loop {rel_err(e_c, e_l):.2e} closed-v1 {rel_err(e_c, e_1):.2e} "
          f"closed-oracle {rel_err(e_c, want):.2e}  {name}")
    assert "eloc_kernel2<" in name
    assert np.count_nonzero(np.abs(want) > 0) > len(keys) // 2
    assert rel_err(e_c, want) <= 1e-10 and rel_err(e_c, e_l) <= 1e-12 and rel_err(e_c, e_1) <= 1e-12
    return closed, e_c


def test_every_pattern_on_one_double_and_one_single(env):
    """No particle-number filter: the keys put all 16 patterns on one double's positions and all 4 on one single's; both
    flip bit 31 of a 32-bit key."""
    N = 32
    rs = np.random.RandomState(41)
    md, ms = (1 << 31) | (1 << 20) | (1 << 9) | (1 << 3), (1 << 31) | (1 << 7)
    keys = set()
    for _ in range(3):
        b = _rand_bits(rs, N) & ~(md | ms) & ((1 << N) - 1)
        keys |= {b | sum(1 << q for i, q in enumerate((3, 9, 20, 31)) if (p >> i) & 1) for p in range(16)}
        keys |= {b | sum(1 << q for i, q in enumerate((7, 31)) if (p >> i) & 1) for p in range(4)}
    keys = np.array(sorted(keys), np.uint64)
    td, ts = d_terms(rs, md, N, 8), s_terms(rs, ms, N, 33)
    xy = np.array([0] * 9 + [md] * len(td) + [ms] * len(ts), np.uint64)
    yz = np.array([_rand_bits(rs, N) for _ in range(9)] + td + ts, np.uint64)
    packed = env["P"].PackedHamiltonian(N, -1, -1, xy, yz, rs.normal(size=len(xy)))
    counts = cr.handle_counts(xy, yz, packed.coeff, N, chunk_terms(packed))
    assert counts[:3] == (1, 1, 0)
    pos_d, pos_s = [3, 9, 20, 31], [7, 31]
    assert {cr.pattern_of(k, pos_d) for k in keys} == set(range(16)) and {cr.pattern_of(k, pos_s) for k in keys} == set(range(4))
    check_synthetic(env, packed, keys, counts)


@pytest.mark.parametrize("filtered", [False, True])
def test_64bit_keys(env, filtered):
    packed, keys, kinds = synthetic(env, 40, 6, 6, 19, filtered=filtered)
    counts = cr.handle_counts(packed.xy, packed.yz, packed.coeff, 40, chunk_terms(packed))
    n_d, n_s = (sum(k == c for k in kinds.values()) for c in "DS")
    # (28 table units per S group at 40 qubits: the last few of ~150 would begin past the word's 12-bit unit field and stay
    # in the loop — the mirror says how many)
    assert counts[0] == n_d > 20 and 20 < counts[1] <= n_s and counts[2] == n_s - counts[1]
    closed, e = check_synthetic(env, packed, keys, counts)
    psi = synth_psi(len(keys), 3)
    assert closed.key_bits == 64 and np.array_equal(run(env, closed, keys, psi), e) and "eloc_kernel2<uint64_t" in closed.last_kernel()
    with environ(NAQS_BLOOM=1, NAQS_BLOCK=1024):
        assert np.array_equal(run(env, closed, keys, psi), e) and "BLOOM=1" in closed.last_kernel()


@pytest.mark.parametrize("N,na,nb", [(32, 8, 8), (40, 6, 6)])
def test_mixed_classes(env, N, na, nb):
    """Qualifying groups beside groups that must fall back: a 4-bit flip where one term carries a spectator, a 2-bit flip
    with a term two spectators away, 6-bit flips — and, with the table bound lowered, groups pushed over it."""
    packed, keys, kinds = synthetic(env, N, na, nb, 23, fallbacks=True)
    chunk = chunk_terms(packed)
    counts = cr.handle_counts(packed.xy, packed.yz, packed.coeff, N, chunk)
    want = tuple(sum(k == c for k in kinds.values()) for c in "DSL")
    assert counts[:3] == want and min(want) >= 5
    six = sum(bin(int(x)).count("1") == 6 for x in np.unique(packed.xy))
    assert six >= 2
    check_synthetic(env, packed, keys, counts)
    # 8 KiB of tables: 64 D groups' worth, no S table fits (4 segments or more: >= 8 KiB + the D slot)
    small = cr.handle_counts(packed.xy, packed.yz, packed.coeff, N, chunk, max_bytes=8 * 1024)
    assert small[1] == 0 and 0 < small[0] <= 64 and small[0] < counts[0] and small[2] > counts[2]
    check_synthetic(env, packed, keys, small, NAQS_CLOSED_MAX_KB=8)


# ------------------------------------------------------------------ nothing may depend on the launch
def test_launch_invariances_n2(env):
    packed = packed_of(env, "N2")
    ham = handle(env, packed, True)
    keys, psi, want = golden_case(env, "N2")[300]
    base = run(env, ham, keys, psi)
    assert "eloc_kernel2<uint32_t, STAGE=2, NT=512, BLOOM=0>" == ham.last_kernel() and rel_err(base, want) <= 1e-10
    seen = {ham.last_kernel()}
    variants = [dict(NAQS_STAGE=s) for s in (0, 1, 2)] + [dict(NAQS_BLOCK=b) for b in (256, 512, 1024)]
    variants += [dict(NAQS_BLOOM=1, NAQS_BLOCK=1024), dict(NAQS_BLOOM=1, NAQS_BLOCK=1024, NAQS_STAGE=0), dict(NAQS_BLOOM=0, NAQS_BLOCK=1024)]
    variants += [dict(NAQS_ROWS_PER_BLOCK=r) for r in (4, 64, 1000)]
    for v in variants:
        with environ(**v):
            assert np.array_equal(run(env, ham, keys, psi), base), v
            seen.add(ham.last_kernel())
    assert len(seen) >= 7, seen
    parts = [run(env, ham, keys, psi, row_begin=len(keys) * r // 3, n_rows=len(keys) * (r + 1) // 3 - len(keys) * r // 3)
             for r in range(3)]
    assert np.array_equal(np.concatenate(parts), base)


def test_fused_call_equals_separate_calls_n2(env):
    from test_nade import make_wf
    from naqs_amd.fused import FusedLogPsi
    z = golden("nade_N2.npz")
    _, wf = make_wf("N2", z, device="cuda")
    fused = FusedLogPsi(wf)
    ham = handle(env, env["P"].load_packed(os.path.join(GOLDEN, "ham_N2.npz")), True)
    assert ham.closed_counts()[:3] == (365, 12, 0)
    keys = env["H"].keys_to_device(z["samp_keys"][:300], wf.device)
    lp = fused.log_psi(keys)
    e = ham.local_energy(keys, lp, kind="log_psi")
    lp2, e2 = fused.log_psi_and_local_energy(ham, keys)
    torch.cuda.synchronize()
    assert torch.equal(lp, lp2) and torch.equal(e, e2)
