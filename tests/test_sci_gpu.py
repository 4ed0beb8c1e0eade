"""Selected CI on the device, every test under both kernel forms of ``naqs_ham_pt2_select`` (NAQS_SELECT_FORM = 1: one workgroup,
one launch; 2: tiles over many workgroups).

* the kernel against the rule restated in NumPy (tests/sci_reference.py: select): the selected keys and both counts
  array_equal, on synthetic rows whose importances make each radix pass decide, with intruders, NaNs, zeros, ties, eps_min,
  tie_rtol, overflow, permutations, repetition and a small call behind a large one;
* on real Hamiltonians (LiH, H2O, a crowded table), the rows of ``pt2(rows=True)``: the rule on the device's own rows exactly,
  and on dense float64 rows at the k whose cut is clear of every other importance (the precondition tests/test_sci.py states)
  and whose rows are decided within their rounding bounds (``decidable``), intruder rows included; the scratch's regrowth;
* the loop ``selected_ci`` against the dense reference loop at the CPU-checked schedules — M equal, |E_S - ref| <= 1e-9 Ha
  (tol = 1e-13: an eigenvalue from a vector of residual r errs by r^2 / gap, far inside), |E_PT2 - ref| <= 1e-8 |E_PT2| + 1e-13,
  both against the dense reference; warm starts; ``v0=None`` bit for bit;
* the optimiser and the command line on LiH.

Observed on one MI355X (profiles/sci.txt): worst |E_S - ref| and |E_PT2 - ref| / |E_PT2| are recorded there."""
import ctypes
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

import pt2_reference as ref
import sci_reference as sci
from conftest import GOLDEN, PKG
from test_eloc_forms_gpu import crowded_tables, naqs_env
from test_eloc_gpu import env  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 2048                       # rows a workgroup of the multi form takes (naqs_select.hip: MULTI_TILE)
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1)
RTOLS = (0.0, 1e-9, 0.5)
FORM_NAME = {1: "select_one_kernel", 2: "select_hist_kernel x8 + select_count_kernel + select_scan_kernel + select_scatter_kernel"}


@pytest.fixture(scope="module", params=[1, 2], autouse=True)
def form(request):
    with naqs_env(SELECT_FORM=request.param):
        yield request.param


@pytest.fixture(scope="module")
def ham(env):
    return env["H"].DevicePauliHamiltonian(env["P"].load_packed(os.path.join(GOLDEN, "ham_LiH.npz")))


def dev(env, keys, device):
    return env["H"].keys_to_device(np.asarray(keys, np.uint64), device)


def host_keys(t):
    return t.cpu().numpy().view(np.uint64)


def device_select(env, ham, keys, num, diag, e0, k, **kw):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), device=ham.device)        # noqa: E731
    sel, n_intr = ham.pt2_select(dev(env, keys, ham.device), t(num), t(diag), e0, k, **kw)
    return host_keys(sel), (int(sel.shape[0]), n_intr)


def agree(env, ham, keys, num, diag, e0, k, **kw):
    got, counts = device_select(env, ham, keys, num, diag, e0, k, **kw)
    want, want_counts, info = sci.select(keys, num, diag, e0, k, **kw)
    assert counts == want_counts and np.array_equal(got, want), (len(keys), k, kw, counts, want_counts)
    return info


# ---- synthetic rows -----------------------------------------------------------------------------------------------------------
def synthetic(pattern, n, seed=0):
    """-> (keys, num, diag, e0 = 0): eps = num^2 / diag.  The patterns whose name starts with 'byte' are exact by construction."""
    rs = np.random.RandomState(seed + n)
    keys = (rs.permutation(4 * n)[:n].astype(np.uint64) + np.uint64(17)) << np.uint64(3)
    j = rs.randint(0, 1 << 30, size=n)
    num, diag = np.ones(n), np.ones(n)
    if pattern == "byte0":                 # 1 / (1 + j 2^-52) = 1 - j 2^-52 exactly for small j: the top seven bytes agree
        diag = 1.0 + (1 + j % 127) * 2.0 ** -52
    elif pattern == "byte7":               # 2^(16 j): only the top byte differs
        num = 2.0 ** (8 * (j % 61 - 30))
    elif pattern == "denormal":            # 2^-(1024 + 2 j)
        num = 2.0 ** -(512.0 + j % 25)
    elif pattern == "equal":
        num, diag = np.full(n, 3.0), np.full(n, 2.0)
    elif pattern == "three":
        num = 1.0 + j % 3
    elif pattern == "mixed":               # every kind of row at once
        num, diag = rs.lognormal(size=n) * rs.choice([-1.0, 1.0], size=n), rs.lognormal(size=n)
        num[j % 4 == 1] = np.round(num[j % 4 == 1], 1)                  # ties
        diag[j % 4 == 1] = 0.5
        kind = rs.randint(0, 16, size=n)
        diag[kind == 0] = -rs.lognormal(size=int((kind == 0).sum()))    # den < 0
        diag[kind == 1] = 0.0                                           # den = 0
        num[kind == 2] = np.nan
        diag[kind == 3] = np.nan
        num[kind == 4] = 0.0
        num[kind == 5] = -0.0
        num[kind == 6] = np.inf
        diag[kind == 7] = np.inf
    else:
        raise ValueError(pattern)
    return keys, num, diag, 0.0


PATTERNS = ("byte0", "byte7", "denormal", "equal", "three", "mixed")


def test_patterns_are_what_they_claim():
    bits = lambda p: sci.importance(*synthetic(p, 1025)[1:])[0].view(np.uint64)         # noqa: E731
    b = bits("byte0")
    assert len(np.unique(b >> np.uint64(8))) == 1 and len(np.unique(b)) > 100
    b = bits("byte7")
    assert len(np.unique(b & np.uint64((1 << 56) - 1))) == 1 and len(np.unique(b >> np.uint64(56))) > 50
    b = bits("denormal")
    assert np.all(b > 0) and np.all(b < np.uint64(1 << 52)) and len(np.unique(b)) == 25
    assert len(np.unique(bits("equal"))) == 1 and len(np.unique(bits("three"))) == 3
    eps, intr, elig = sci.importance(*synthetic("mixed", 1025)[1:])
    assert intr.sum() > 100 and (~elig).sum() > 50 and np.isinf(eps[~intr]).any()


def ks_for(eps, eligible, n):
    s = np.sort(eps[eligible])[::-1]
    ks = {0, 1, max(1, len(s) // 2), n - 1, n, n + 5, -2}
    same = np.flatnonzero(s[1:] == s[:-1])
    if len(same):
        ks.add(int(same[0]) + 1)                        # the k-th and the (k+1)-th tie: inside a group
        ks.add(int(same[len(same) // 2]) + 1)
    step = np.flatnonzero(s[1:] != s[:-1])
    if len(step):
        ks.add(int(step[0]) + 1)                        # a group's last member
        ks.add(int(step[0]) + 2)                        # the next group's first
        ks.add(int(step[len(step) // 2]) + 1)
    return sorted(ks)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_kernel_against_the_rule(env, ham, form, pattern):
    n_calls = 0
    for n in SIZES:
        keys, num, diag, e0 = synthetic(pattern, n)
        eps, intr, elig = sci.importance(num, diag, e0)
        for k in ks_for(eps, elig, n):
            for rtol in RTOLS:
                info = agree(env, ham, keys, num, diag, e0, k, tie_rtol=rtol)
                n_calls += 1
            if info["tau"] is not None and np.isfinite(info["tau"]):
                # eps_min below tau, at tau (>= keeps it) and above it
                for eps_min in (float(info["tau"]) * 0.5, float(info["tau"]), float(np.nextafter(info["tau"], np.inf))):
                    agree(env, ham, keys, num, diag, e0, k, eps_min=eps_min)
                    n_calls += 1
        assert ham.last_kernel() == FORM_NAME[form]
    print(f"{pattern} form {form}: {n_calls} calls")


def test_more_than_one_tile_and_the_scan(env, ham, form):
    """Five tiles and a row: the offsets of the multi form's scan, the strided loops of the one-workgroup form."""
    n = 5 * TILE + 1
    for pattern in ("mixed", "three"):
        keys, num, diag, e0 = synthetic(pattern, n)
        eps, intr, elig = sci.importance(num, diag, e0)
        for k in (1, 100, int(elig.sum()) // 2, int(elig.sum()) - 1, n):
            agree(env, ham, keys, num, diag, e0, k)


def test_permutation_repetition_and_a_small_call_after_a_large_one(env, ham, form):
    keys, num, diag, e0 = synthetic("mixed", 3 * TILE + 5)
    k = 700
    first, counts = device_select(env, ham, keys, num, diag, e0, k)
    again, counts2 = device_select(env, ham, keys, num, diag, e0, k)
    assert np.array_equal(first, again) and counts == counts2
    p = np.random.RandomState(9).permutation(len(keys))
    perm, counts3 = device_select(env, ham, keys[p], num[p], diag[p], e0, k)
    assert counts3 == counts and np.array_equal(np.sort(perm), np.sort(first)) and np.array_equal(perm, keys[p][np.isin(keys[p], first)])
    small = synthetic("three", 65)
    got = device_select(env, ham, *small, 7)
    fresh = env["H"].DevicePauliHamiltonian(env["P"].load_packed(os.path.join(GOLDEN, "ham_LiH.npz")))
    want = device_select(env, fresh, *small, 7)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    agree(env, ham, *small, 7)


def test_scratch_regrowth(env, form):
    """The multi form's scratch starts at 64 tiles (131 072 rows) and is released and allocated anew beyond: a call inside it, one
    past it, and a small one behind that, each against the rule, on a handle of their own."""
    h = env["H"].DevicePauliHamiltonian(env["P"].load_packed(os.path.join(GOLDEN, "ham_LiH.npz")))
    for pattern, n, k in (("three", 65, 7), ("mixed", 64 * TILE + 1, 5000), ("three", 65, 7), ("mixed", 3 * TILE + 5, 700), ("byte0", 200 * TILE - 3, 99999)):
        keys, num, diag, e0 = synthetic(pattern, n)
        agree(env, h, keys, num, diag, e0, k)
        assert h.last_kernel() == FORM_NAME[form]


def raw(env, ham, keys, num, diag, e0, k, eps_min, rtol, capacity, n_out):
    kd = dev(env, keys, ham.device)
    nd, dd = (torch.as_tensor(np.asarray(a, np.float64), device=ham.device) for a in (num, diag))
    out = torch.full((n_out,), -1, dtype=torch.int64, device=ham.device)
    count = torch.full((2,), -7, dtype=torch.int64, device=ham.device)
    n = len(keys)
    st = env["lib"].load_library().naqs_ham_pt2_select(ham._h, n, kd.data_ptr() if n else None, nd.data_ptr() if n else None,
                                                       dd.data_ptr() if n else None, e0, k, eps_min, rtol, capacity,
                                                       out.data_ptr() if n_out else None, count.data_ptr(),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), count.cpu().numpy()


def test_overflow_empty_and_invalid(env, ham, form):
    keys, num, diag, e0 = synthetic("mixed", TILE + 77)
    want, (n_sel, n_intr), _ = sci.select(keys, num, diag, e0, 300)
    assert n_sel >= 300
    st, out, count = raw(env, ham, keys, num, diag, e0, 300, 0.0, 1e-9, n_sel - 1, n_sel + 16)
    assert st == 0 and list(count) == [n_sel, n_intr] and np.all(out[n_sel - 1:] == -1)         # counted, nothing behind the capacity
    st, out, count = raw(env, ham, keys, num, diag, e0, 300, 0.0, 1e-9, 0, 0)
    assert st == 0 and list(count) == [n_sel, n_intr]
    st, out, count = raw(env, ham, keys, num, diag, e0, 300, 0.0, 1e-9, n_sel, n_sel + 16)
    assert st == 0 and list(count) == [n_sel, n_intr] and np.array_equal(out[:n_sel].view(np.uint64), want) and np.all(out[n_sel:] == -1)
    st, out, count = raw(env, ham, keys[:0], num[:0], diag[:0], e0, 5, 0.0, 1e-9, 0, 0)
    assert st == 0 and list(count) == [0, 0]
    sel, n_intr0 = ham.pt2_select(dev(env, keys[:0], ham.device), torch.zeros(0), torch.zeros(0), e0, 5)
    assert sel.shape == (0,) and n_intr0 == 0
    for eps_min, rtol, e in ((-1.0, 0.0, e0), (0.0, -1e-9, e0), (float("nan"), 0.0, e0), (0.0, float("nan"), e0), (0.0, 0.0, float("nan")),
                             (0.0, 0.0, float("inf"))):
        st, out, count = raw(env, ham, keys, num, diag, e, 300, eps_min, rtol, len(keys), len(keys))
        assert st == -1 and list(count) == [-7, -7]


# ---- real Hamiltonians ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def molecule_abs(mol):
    packed, keys = ref.molecule(mol)[:2]
    return ref.dense_abs(packed, keys)


def decidable(num, err, den, den_err, k, tie_rtol=1e-9):
    """May the dense rows and the device's be asked for the same selection at this k?  Both sides round a row's numerator (a sum
    that may cancel: LiH from one determinant has numerators of 2e-10 left over from terms of 1e-2) within ``err`` = (groups)
    2^-53 sum |terms| — the bound tests/test_pt2_gpu.py holds the kernel to — and its denominator within ``den_err``; a row's
    numerator is therefore uncertain by 2 err between them and its denominator by 2 den_err.  The conditions:
    (o)   every row's intruder status is decided: |den| > 2 den_err.  An intruder is then an intruder on both sides (eps = +inf,
          always among the first selected);
    (i)   tests/test_sci.py's precondition at a finite cut: no importance within 1e-6 of it but tau's own group (within 1e-12);
    (ii)  the rows stay where (i) found them.  A row above the group stays above cut (1 + 1e-8) with (|num| - 2 err)^2 over
          den + 2 den_err, a row below stays below cut (1 - 1e-8) with (|num| + 2 err)^2 over den - 2 den_err: the three sets
          keep their ranks, so the k-th largest is still a member of the group.  A member's importance carries a relative
          uncertainty d = 2 (2 err) / |num| + 2 den_err / den; every member must still reach the cut formed from any other,
          (1 - 1e-12 - d) >= (1 + 1e-12 + d) (1 - tie_rtol), i.e. d <= (tie_rtol - 2e-12) / 2 to first order: d <= 4e-10 is asked;
    (iii) k at or beyond the number of eligible rows selects them all: every row's eligibility must be decided, a numerator
          either clear of its rounding (|num| > 2 err) or with no term at all (err = 0)."""
    if k <= 0:
        return True
    if np.any(np.isnan(num) | ~(np.abs(den) > 2.0 * den_err)):
        return False
    eps, intruder, eligible = sci.importance(num, den, 0.0)
    s = np.sort(eps[eligible])
    if k >= len(s):
        return bool(np.all(intruder | (np.abs(num) > 2.0 * err) | (err == 0)))
    tau = s[len(s) - k]
    if np.isinf(tau):                     # the cut lies among the intruders: they all tie, nothing else reaches +inf
        return True
    cut = tau * (1.0 - tie_rtol)
    if tie_rtol < 1e-9 or sci.cuts_are_clear([dict(eps=eps, tau=tau, cut=cut)]) != []:
        return False
    finite = ~intruder
    group = finite & (np.abs(eps - tau) <= 1e-12 * tau)
    above, below = finite & ~group & (eps >= cut), finite & ~group & (eps < cut)
    lo = np.maximum(np.abs(num) - 2.0 * err, 0.0) ** 2 / (den + 2.0 * den_err)
    hi = (np.abs(num) + 2.0 * err) ** 2 / (den - 2.0 * den_err)
    d = 4.0 * err[group] / np.abs(num[group]) + 2.0 * den_err / den[group]
    return bool(np.all(lo[above] > cut * (1.0 + 1e-8)) and np.all(hi[below] < cut * (1.0 - 1e-8)) and np.all(d <= 4e-10))


def rounding(packed, e0):
    """-> (groups 2^-53: the factor of a numerator's bound; the bound of a denominator's error: the diagonal's terms and the
    subtraction, (terms + 1) 2^-53 (sum |coeff| + |e0|))."""
    n_diag = int(np.sum(np.asarray(packed.xy) == 0))
    return len(np.unique(packed.xy)) * 2.0 ** -53, (n_diag + 1) * 2.0 ** -53 * (ref.diag_bound(packed) + abs(e0))


def compare(ham, ext, num, diag, rows, num_d, diag_d, err, den_err, e0, ks, tag):
    """The device's selection at every k against the rule on its own rows (always) and on the dense rows (where decidable).
    -> (dense comparisons made, of which with intruders among the rows)."""
    num_h, diag_h = num.cpu().numpy(), diag.cpu().numpy()
    n_dense = 0
    for k in ks:
        sel, n_intr = ham.pt2_select(ext, num, diag, e0, k)
        mine = sci.select(rows, num_h, diag_h, e0, k)
        assert np.array_equal(host_keys(sel), mine[0]) and (int(sel.shape[0]), n_intr) == mine[1], (tag, k)
        if decidable(num_d, err, diag_d - e0, den_err, k):
            dense = sci.select(rows, num_d, diag_d, e0, k)
            assert np.array_equal(host_keys(sel), dense[0]) and (int(sel.shape[0]), n_intr) == dense[1], (tag, k)
            n_dense += 1
    return n_dense


@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_rows_of_real_molecules(env, form, mol):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    ham = env["H"].DevicePauliHamiltonian(packed)
    n_dense = n_with_intruders = 0
    for S in (ref.top_S(H, 1), ref.top_S(H, 16), ref.top_S(H, 40), ref.random_S(len(keys), 17, 7), ref.random_S(len(keys), 60, 8)):
        e0, c = ref.ground(H, S)
        kd = dev(env, keys[S], ham.device)
        ext, n_ext = ham.connected_keys(kd)
        out4, num, diag = ham.pt2(kd, torch.as_tensor(c, device=ham.device), e0, ext, rows=True)
        rows = host_keys(ext)
        want = ref.pt2(H, S, c, e0)
        at = np.searchsorted(keys[want["ext"]], rows)
        num_d, diag_d = want["r"][at], want["diag"][at]                 # the dense rows of the connected set
        factor, den_err = rounding(packed, e0)
        err = factor * (molecule_abs(mol)[np.ix_(want["ext"][at], S)] @ np.abs(c))
        n = compare(ham, ext, num, diag, rows, num_d, diag_d, err, den_err, e0,
                    (0, 1, 2, 3, 5, 8, 13, 21, 34, n_ext // 2, n_ext - 1, n_ext, n_ext + 3), (mol, len(S)))
        n_dense += n
        n_with_intruders += n if np.any(~(diag_d - e0 > 0)) else 0
    assert n_dense >= 50 and n_with_intruders >= 10                     # the random subspaces have external states below E_S
    print(f"{mol} form {form}: {n_dense} selections equal to the dense float64 rows', {n_with_intruders} of them with intruders among the rows")


def test_rows_of_a_crowded_table(env, form):
    """The crowded table of tests/test_eloc_forms.py (512 keys on one home slot), random coefficients.  Its whole connected set
    (1.5e5 rows) against the rule on the device's own rows; 3 000 of those rows, in random order, also against dense float64
    rows from the definition (sci_reference.block / diagonal).  Nearly half the rows are intruders at either e0, so the k of
    interest lie beyond their number."""
    from naqs_amd.packing import PackedHamiltonian
    packed, tabs = crowded_tables(32)
    keys = np.asarray(tabs["A"][0], np.uint64)
    ham = env["H"].DevicePauliHamiltonian(packed)
    c = np.random.RandomState(71).normal(size=len(keys))
    c /= np.linalg.norm(c)
    kd, cd = dev(env, keys, ham.device), torch.as_tensor(c, device=ham.device)
    ext, n_ext = ham.connected_keys(kd)
    assert n_ext > 1024
    sub = host_keys(ext)[np.random.RandomState(5).permutation(n_ext)[:3000]]
    sub_d = dev(env, sub, ham.device)
    num_d, diag_d = sci.block(packed, sub, keys) @ c, sci.diagonal(packed, sub)
    magnitudes = PackedHamiltonian(packed.n_qubits, packed.n_alpha, packed.n_beta, packed.xy, np.zeros_like(packed.yz), np.abs(packed.coeff))
    bound = sci.block(magnitudes, sub, keys) @ np.abs(c)
    n_dense = n_beyond = 0
    for e0 in (-1.0, 0.25):                                               # rows on both sides of the denominator's sign at either
        out4, num, diag = ham.pt2(kd, cd, e0, ext, rows=True)
        rows, num_h, diag_h = host_keys(ext), num.cpu().numpy(), diag.cpu().numpy()
        for k in (1, 50, n_ext // 3, n_ext - 1, n_ext):
            sel, n_intr = ham.pt2_select(ext, num, diag, e0, k)
            mine = sci.select(rows, num_h, diag_h, e0, k)
            assert np.array_equal(host_keys(sel), mine[0]) and (int(sel.shape[0]), n_intr) == mine[1], (e0, k)
        out4, num, diag = ham.pt2(kd, cd, e0, sub_d, rows=True)
        n_i = int(np.sum(~(diag_d - e0 > 0)))
        assert 100 < n_i < len(sub) - 100
        factor, den_err = rounding(packed, e0)
        beyond = (n_i + 1, n_i + 2, n_i + 7, n_i + 30, n_i + 100, n_i + 300, n_i + 1000, (n_i + len(sub)) // 2)
        n_beyond += compare(ham, sub_d, num, diag, sub, num_d, diag_d, factor * bound, den_err, e0, beyond, ("crowded", e0))
        n_dense += compare(ham, sub_d, num, diag, sub, num_d, diag_d, factor * bound, den_err, e0, (1, n_i, len(sub) - 1, len(sub)), ("crowded", e0))
    assert n_beyond >= 14 and n_dense >= 6
    print(f"crowded form {form}: {n_beyond + n_dense} selections equal to the dense float64 rows', {n_beyond} of them cut among the finite importances "
          f"behind the intruders")


# ---- the loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", ["LiH", "H2O", "N2"])
def test_loop_against_the_dense_reference(env, form, mol):
    packed, fci, k0 = sci.start(mol)
    want = sci.loop(packed, k0, sci.SCHEDULES[mol])
    ham = env["H"].DevicePauliHamiltonian(packed)
    got = ham.selected_ci(dev(env, k0, ham.device), sci.SCHEDULES[mol], tol=1e-13)
    assert got["stopped"] == want["stopped"] == "schedule" and len(got["history"]) == len(want["history"])
    worst_e = worst_p = 0.0
    for g, w in zip(got["history"], want["history"]):
        assert (g["M"], g["n_external"], g["n_intruders"], g["n_added"]) == (w["M"], w["n_external"], w["n_intruders"], w["n_added"])
        worst_e = max(worst_e, abs(g["e0"] - w["e0"]))
        worst_p = max(worst_p, abs(g["e_pt2"] - w["e_pt2"]) / abs(w["e_pt2"]))
    print(f"{mol} form {form}: M {[g['M'] for g in got['history']]}, worst |E_S - ref| {worst_e:.2e} Ha, "
          f"worst |E_PT2 - ref| / |E_PT2| {worst_p:.2e}")
    for g, w in zip(got["history"], want["history"]):
        assert abs(g["e0"] - w["e0"]) <= 1e-9
        assert abs(g["e_pt2"] - w["e_pt2"]) <= 1e-8 * abs(w["e_pt2"]) + 1e-13
    assert np.array_equal(host_keys(got["keys"]), want["keys"])
    assert got["extrapolated"] == pytest.approx(env["H"].extrapolate_pt2(want["history"]), abs=1e-7)
    assert abs(float(got["vec"].norm()) - 1.0) < 1e-12 and got["vec"].shape[0] == want["history"][-1]["M"]


@pytest.mark.parametrize("mol", ["LiH", "N2"])
def test_warm_start_and_the_old_start(env, form, mol):
    packed, fci, k0 = sci.start(mol)
    want = sci.loop(packed, k0, sci.SCHEDULES[mol])
    ham = env["H"].DevicePauliHamiltonian(packed)
    sizes = [h["M"] for h in want["history"]]
    all_keys = dev(env, want["keys"], ham.device)
    for small, large in list(zip(sizes, sizes[1:]))[-3:]:
        e_small, c = ham.lowest_eigenpair(all_keys[:small], tol=1e-10)
        kd = all_keys[:large].contiguous()
        e_cold, v_cold = ham.lowest_eigenpair(kd, tol=1e-10)
        cold = ham.last_lanczos_iterations
        v0 = torch.cat([c, torch.zeros(large - small, dtype=torch.float64, device=ham.device)])
        e_warm, v_warm = ham.lowest_eigenpair(kd, tol=1e-10, v0=v0)
        warm = ham.last_lanczos_iterations
        print(f"{mol} {small} -> {large}: {cold} products cold, {warm} warm")
        assert warm <= cold and abs(e_warm - e_cold) <= 1e-9 and e_warm <= e_small + 1e-12
        # v0 = None is the call as it was; the seeded start handed over by the caller lands on the same bits
        e_none, v_none = ham.lowest_eigenpair(kd, 400, 1e-10, 0)
        assert e_none == e_cold and torch.equal(v_none, v_cold)
        gen = torch.Generator(device=ham.device).manual_seed(0)
        start = torch.randn(large, dtype=torch.float64, device=ham.device, generator=gen)
        e_same, v_same = ham.lowest_eigenpair(kd, tol=1e-10, v0=start)
        assert e_same == e_cold and torch.equal(v_same, v_cold)
    with pytest.raises(ValueError):
        ham.lowest_eigenpair(all_keys[:4], v0=torch.zeros(4, dtype=torch.float64, device=ham.device))


def test_early_stops(env, form):
    packed, fci, k0 = sci.start("LiH")
    ham = env["H"].DevicePauliHamiltonian(packed)
    res = ham.selected_ci(dev(env, k0, ham.device), (1000,) * 8, tol=1e-13)
    last = res["history"][-1]
    assert res["stopped"] == "connected set empty" and last["M"] == 69 and last["n_external"] == 0 and abs(last["e0"] - fci) <= 1e-9
    res = ham.selected_ci(dev(env, k0, ham.device), (1, 2, 4, 8), max_states=6)
    assert res["stopped"] == "max_states" and [h["M"] for h in res["history"]] == [1, 2, 4] and res["keys"].shape[0] == 4
    res = ham.selected_ci(dev(env, k0, ham.device), (1, 2, 4, 8), eps_min=1e3)
    assert res["stopped"] == "nothing eligible" and len(res["history"]) == 1 and res["extrapolated"] is None
    res = ham.selected_ci(dev(env, k0, ham.device), (3, 1.0))
    assert [h["M"] for h in res["history"]] == [1, 2, 4] and res["stopped"] == "schedule"


# ---- the optimiser and the command line -------------------------------------------------------------------------------------
def test_solve_h_sci_starts_where_solve_h_pt2_stands(env, form, tmp_path):
    from test_exact_eloc_gpu import _net, _opt
    hil, wf = _net("LiH", fallback=False)
    opt = _opt("LiH", wf, tmp_path)
    state, calls = opt.generator.get_state(), wf._sample_calls
    one = opt.solve_H_pt2(n_samps=100000)
    after = (opt.generator.get_state(), wf._sample_calls)
    opt.generator.set_state(state)
    wf._sample_calls = calls
    got = opt.solve_H_sci(n_samps=100000, n_iter=3, grow=0.5)
    assert torch.equal(opt.generator.get_state(), after[0]) and wf._sample_calls == after[1] == calls + 1
    h0 = got["history"][0]
    assert (h0["e0"], h0["e_pt2"], h0["n_external"], h0["n_intruders"], got["n_unq"]) == \
        (one["eig"], one["e_pt2"], one["n_external"], one["n_intruders"], one["n_unq"])               # bit for bit
    e = [h["e0"] for h in got["history"]]
    assert all(b <= a + 1e-12 for a, b in zip(e, e[1:]))
    assert got["stopped"] in ("schedule", "connected set empty", "nothing eligible") and (len(e) == 3) == (got["stopped"] == "schedule")
    opt.generator.set_state(state)
    wf._sample_calls = calls
    cut = opt.solve_H_sci(n_samps=100000, n_iter=2, n_start=5)
    assert cut["history"][0]["M"] == 5 and cut["n_unq"] == one["n_unq"] and opt.solve_H_max_states == 10000
    assert cut["history"][1]["M"] >= 10


def test_sci_flags_of_the_command_line(form, tmp_path, capsys):
    sys.path.insert(0, PKG)
    from experiments import _base
    common = ["-m", os.path.join(GOLDEN, "ham_LiH.npz"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_layer_phase", "2",
              "-n_samps", "100000", "-n_unq_samps_min", "10", "-n_unq_samps_max", "100000", "-n_train", "6", "-output_freq", "2",
              "-lr", "0.001", "-s", "7"]
    res = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "on"), "-sci", "3", "-sci_start", "12"])
    out = capsys.readouterr().out
    summary = open(tmp_path / "on" / "summary.txt").read().splitlines()
    its = [ln for ln in summary if ln.startswith("selected CI iteration ")]
    assert len(its) == 3 and its[0].startswith("selected CI iteration 0 (12 states, ") and all("mHa" in ln for ln in its)
    assert summary[-1].startswith("selected CI stopped : ") and all(ln in out for ln in its)
    assert "\tsci : 3" in out and "\tsci_start : 12" in out and "sci_grow" not in out
    assert not any("Epstein-Nesbet PT2" in ln for ln in summary)                         # that line is -pt2's
    r = res[0]
    hist = r["sci_history"]
    with capsys.disabled():
        print(f"\nLiH after 6 steps: E_S - FCI {[round((h['e0'] - r['fci']) * 1e3, 4) for h in hist]} mHa at M {[h['M'] for h in hist]}")
    assert hist[-1]["e0"] <= hist[0]["e0"] and r["eig"] == hist[0]["e0"] and hist[-1]["e0"] >= r["fci"] - 1e-9
    sub = [ln for ln in summary if ln.startswith("sampled-subspace diagonalisation (")]
    assert len(sub) == 1 and sub[0].endswith(f": {hist[0]['e0']:.8f}")
    res = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "off")])
    out = capsys.readouterr().out
    assert "selected CI" not in out and "\tsci" not in out and "selected CI" not in open(tmp_path / "off" / "summary.txt").read()
    assert not any(k.startswith("sci") for k in res[0])
