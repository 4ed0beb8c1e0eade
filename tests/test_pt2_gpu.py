"""``naqs_ham_pt2`` on the MI355X: the rows (num, diag) against the dense float64 reference of tests/pt2_reference.py on the LiH
and H2O fixtures, the four sums against exactly rounded sums of the device's own rows, every kernel instance the dispatcher
can form on the Hamiltonians of tests/test_eloc_forms.py (names asserted, bits equal across forms, table order, row order and
row count, agreement with ``naqs_hmatvec`` on the union table), rows that are table rows, the argument checks, and a short
``experiments.run -pt2``.

Bounds: a row within 1e-10 max(1, sum_j (sum_{t in group} |coeff_t|) |c_j|) of the reference (the E_loc bound of
tests/test_eloc_gpu.py); a sum within n 2^-53 sum |terms| of the exact sum of the device's rows ((n - 1) 2^-53 is the a-priori
bound of any summation order, and the kernel forms each term num^2 / (e0 - diag) to one rounding; the smallest set here has
four rows); E_PT2 within 1e-10 sum |terms| of the reference; 1e-12 max(1, |want|) against the union-table product, whose
partial sums are grouped differently.
"""
import ctypes
import os
import sys
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

import pt2_reference as ref
import test_eloc_forms as F
from conftest import GOLDEN, PKG
from test_eloc_forms_gpu import crowded_tables, heavy_case, naqs_env
from test_eloc_gpu import env  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOP_M = (1, 3, 63, 64, 65, 200)
RANDOM_M = (17, 65, 130)
INVALID, UNSUPPORTED = -1, -4


def dev(env, keys, device):
    return env["H"].keys_to_device(np.asarray(keys, np.uint64), device)


def host_keys(t):
    return t.cpu().numpy().view(np.uint64)


def call(ham, kd, c, e0, ext, rows=True):
    out = ham.pt2(kd, torch.as_tensor(np.asarray(c, np.float64), device=ham.device), e0, ext, rows=rows)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if rows else out.cpu().numpy()


def exact_sums(num, diag, e0):
    """The four sums of the rows, and the sums of their terms' magnitudes, in rational arithmetic on the doubles."""
    sums, mags = [Fraction(0)] * 4, [Fraction(0)] * 4
    for n, d in zip(num, diag):
        n, d = Fraction(float(n)), Fraction(float(d))
        den = Fraction(float(e0)) - d
        if den < 0:
            terms = ((0, n * n / den), (1, n * n))
        else:
            terms = ((2, Fraction(1)), (3, n * n))
        for k, t in terms:
            sums[k] += t
            mags[k] += abs(t)
    return sums, mags


@lru_cache(maxsize=None)
def molecule_abs(mol):
    packed, keys = ref.molecule(mol)[:2]
    return ref.dense_abs(packed, keys)


def subspaces(mol):
    n = len(ref.molecule(mol)[1])
    H = ref.molecule(mol)[2]
    for M in TOP_M:
        yield "top", M, ref.top_S(H, M)
    for M in RANDOM_M:
        yield "random", M, ref.random_S(n, M, 7)


# ---- per row and the sums, real molecules ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_rows_and_sums_against_the_dense_reference(env, mol):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    Habs = molecule_abs(mol)
    ham = env["H"].DevicePauliHamiltonian(packed)
    dbound = ref.diag_bound(packed)
    worst = dict(num=0.0, diag=0.0, sums=0.0, e_pt2=0.0)
    for kind, M, S in subspaces(mol):
        e_s, c_s = ref.ground(H, S)
        rs = np.random.RandomState(100 + M)
        c_r = rs.normal(size=M)
        c_r /= np.linalg.norm(c_r)
        kd = dev(env, keys[S], ham.device)
        ext, n_ext = ham.connected_keys(kd)
        ext_h = host_keys(ext)
        assert np.array_equal(ext_h, ref.connected_set(packed, keys[S])) and n_ext == len(ext_h) >= 4
        for tag, c, e0 in (("eigenvector", c_s, e_s), ("random", c_r, float(c_r @ H[np.ix_(S, S)] @ c_r))):
            want = ref.pt2(H, S, c, e0)
            at = np.searchsorted(keys[want["ext"]], ext_h)
            assert np.array_equal(keys[want["ext"]][at], ext_h)
            # every sector key outside S that is not in the connected set has r = 0 in the reference
            off = np.ones(len(want["ext"]), bool)
            off[at] = False
            assert np.all(want["r"][off] == 0.0)
            out4, num, diag = call(ham, kd, c, e0, ext)
            assert ham.last_kernel().startswith("pt2_kernel<uint32_t, STAGE=2, NT=512")
            bound = 1e-10 * np.maximum(1.0, Habs[np.ix_(want["ext"][at], S)] @ np.abs(c))
            err_n, err_d = np.abs(num - want["r"][at]), np.abs(diag - want["diag"][at])
            worst["num"] = max(worst["num"], float(np.max(err_n / bound)))
            worst["diag"] = max(worst["diag"], float(np.max(err_d)) / (1e-10 * max(1.0, dbound)))
            assert np.all(err_n <= bound), (mol, kind, M, tag, float(np.max(err_n / bound)))
            assert np.all(err_d <= 1e-10 * max(1.0, dbound)), (mol, kind, M, tag, float(np.max(err_d)))
            # the sums: exactly rounded sums of the device's own rows
            exact, mags = exact_sums(num, diag, e0)
            for k in range(4):
                err, lim = abs(Fraction(float(out4[k])) - exact[k]), n_ext * Fraction(1, 2 ** 53) * mags[k]
                if mags[k]:
                    worst["sums"] = max(worst["sums"], float(err / lim))
                assert err <= lim, (mol, kind, M, tag, k, float(err), float(lim))
            # ... and the reference's: E_PT2, the intruders' count and their residual
            # (the reference sums over ALL states outside S; one that no term connects to S has r = 0 and adds to no sum, but it
            # is counted when it lies below e0: the count is compared over the connected rows, which is what the call is given)
            den = e0 - want["diag"][at]
            n_intruders = int(np.sum(~(den < 0)))
            assert n_intruders <= want["n_intruders"]
            terms = float(np.sum(np.abs(want["r"][at] ** 2 / den)[den < 0]))
            worst["e_pt2"] = max(worst["e_pt2"], abs(out4[0] - want["e_pt2"]) / max(1e-10 * terms, 1e-300))
            assert abs(out4[0] - want["e_pt2"]) <= 1e-10 * terms, (mol, kind, M, tag, out4[0], want["e_pt2"])
            assert abs(out4[1] - want["residual2"]) <= 1e-10 * max(1.0, want["residual2"])
            if np.min(np.abs(den)) > 1e-9:                                   # (a denominator at zero has no side)
                assert int(out4[2]) == n_intruders, (mol, kind, M, tag)
                assert abs(out4[3] - want["intruder_residual2"]) <= 1e-10 * max(1.0, want["intruder_residual2"])
            if kind == "random" and tag == "eigenvector":
                assert n_intruders > 0 and np.min(np.abs(den)) > 1e-9 and int(out4[2]) == n_intruders
                assert out4[0] <= 0.0                                        # their (positive) terms are absent from [0]
            if kind == "top" and tag == "eigenvector":
                assert out4[2] == 0.0 and out4[3] == 0.0
    print(f"{mol}: worst error / bound: num {worst['num']:.3e}, diag {worst['diag']:.3e}, sums {worst['sums']:.3f}, E_PT2 {worst['e_pt2']:.3e}")


def test_the_correction_on_the_device(env):
    """pt2_correction end to end on the fixtures: the table of the issue, with the device's Lanczos vector."""
    for mol, M, gain in (("LiH", 17, 1e-6), ("H2O", 63, 1e-7)):
        packed, keys, H, w, v, fci = ref.molecule(mol)
        S = ref.top_S(H, M)
        ham = env["H"].DevicePauliHamiltonian(packed)
        kd = dev(env, keys[S], ham.device)
        e0, vec = ham.lowest_eigenpair(kd)
        res = ham.pt2_correction(kd, vec)
        want = ref.pt2(H, S, *ref.ground(H, S)[::-1])
        assert set(res) == {"e0", "e_pt2", "n_external", "n_intruders", "residual2", "intruder_residual2"}
        assert abs(res["e0"] - e0) < 1e-9 and res["n_intruders"] == 0 and res["n_external"] == len(ref.connected_set(packed, keys[S]))
        assert abs(res["e_pt2"] - want["e_pt2"]) < 1e-9 and abs(e0 + res["e_pt2"] - fci) < gain
        with pytest.raises(ValueError, match=rf"{ham.connected_capacity(M, M)}.*max_external = 5"):
            ham.pt2_correction(kd, vec, max_external=5)
    # the whole sector: no external key
    kd = dev(env, keys, ham.device)
    e0, vec = ham.lowest_eigenpair(kd)
    res = ham.pt2_correction(kd, vec, e0=e0)
    assert res["n_external"] == 0 and res["e_pt2"] == 0.0 and res["n_intruders"] == 0


# ---- every instance --------------------------------------------------------------------------------------------------------
def expected_name(packed, n_rows, block=None, stage=2, filter_built=False):
    kb = 32 if packed.n_qubits <= 32 else 64
    nt = block or F.default_block(n_rows)
    bloom = bool(filter_built) and nt == 1024
    return F.kernel_name(kb, True, min(stage, F.natural_stage(packed, nt, True, bloom)), nt, bloom).replace("eloc_kernel2", "pt2_kernel")


def instance_cases():
    for kind in ("f32", "u32", "f64", "u64"):
        yield kind
    yield "crowded32"
    yield "crowded64"


@lru_cache(maxsize=None)
def instance_case(kind):
    """-> (packed, table keys, coefficients): heavy_case's 1 499 keys, the crowded table's 512."""
    if kind.startswith("crowded"):
        packed, tabs = crowded_tables(int(kind[-2:]))
        keys = tabs["A"][0]
    else:
        packed, keys = heavy_case(kind)[:2]
    c = np.random.RandomState(71).normal(size=len(keys))
    return packed, np.asarray(keys, np.uint64), c / np.linalg.norm(c)


@pytest.mark.parametrize("kind", list(instance_cases()))
def test_every_instance(env, kind):
    packed, keys, c = instance_case(kind)
    kb = 32 if packed.n_qubits <= 32 else 64
    ham = env["H"].DevicePauliHamiltonian(packed)
    M = len(keys)
    kd = dev(env, keys, ham.device)
    conn, n_conn = ham.connected_keys(kd)
    rs = np.random.RandomState(3)
    # at most 1 500 rows, in random order; with the crowded table the absent half of its pool among them
    rows = host_keys(conn)
    pick = rs.permutation(len(rows))[:1500]
    if kind.startswith("crowded"):
        pool_b = crowded_tables(kb)[1]["B"][0]
        pick = np.union1d(pick[:1200], np.flatnonzero(np.isin(rows, pool_b)))
        assert np.isin(rows[pick], pool_b).sum() >= 100
    rows = rows[rs.permutation(pick)]
    n = len(rows)
    assert n >= 1024 and len(np.intersect1d(rows, keys)) == 0
    rd = dev(env, rows, ham.device)
    e0 = -1.0
    seen = set()
    first = None
    for stage in (2, 0):
        for block in (None, 512, 1024):
            for bloom in (0, 1):
                with naqs_env(STAGE=stage, BLOCK=block, BLOOM=bloom):
                    out4, num, diag = call(ham, kd, c, e0, rd)
                name = ham.last_kernel()
                assert name == expected_name(packed, n, block, stage, bloom), (kind, stage, block, bloom)
                seen.add(name)
                if first is None:
                    first = (out4, num, diag)
                assert np.array_equal(num, first[1]) and np.array_equal(diag, first[2]) and np.array_equal(out4, first[0]), name
    assert len(seen) == 6 and sum("BLOOM=1" in s for s in seen) == 2
    out4, num, diag = first
    assert np.count_nonzero(num) > 0.9 * n and (packed.n_alpha < 0 or np.count_nonzero(diag) == n)
    # a permutation of the table, c with it
    perm = rs.permutation(M)
    _, num_p, diag_p = call(ham, dev(env, keys[perm], ham.device), c[perm], e0, rd)
    assert np.array_equal(num_p, num) and np.array_equal(diag_p, diag)
    # a permutation of the rows, the outputs with it
    perm = rs.permutation(n)
    out4_p, num_p, diag_p = call(ham, kd, c, e0, dev(env, rows[perm], ham.device))
    assert np.array_equal(num_p, num[perm]) and np.array_equal(diag_p, diag[perm])
    # row counts around the waves of each form
    for block in (None, 512, 1024):
        for m in sorted({1, n} | {(block or F.default_block(1)) // F.WAVE + d for d in (-1, 0, 1)}):
            with naqs_env(BLOCK=block):
                _, num_m, diag_m = call(ham, kd, c, e0, rd[:m])
            assert ham.last_kernel() == expected_name(packed, m, block)
            assert np.array_equal(num_m, num[:m]) and np.array_equal(diag_m, diag[:m]), (block, m)
    # the parent's route to the same numbers: the union table through naqs_hmatvec, v = (c, 0)
    union = torch.cat([kd, rd])
    v = torch.cat([torch.as_tensor(c, device=ham.device), torch.zeros(n, dtype=torch.float64, device=ham.device)])
    want = ham.matvec(union, v)[M:].cpu().numpy()
    err = np.max(np.abs(num - want) / np.maximum(1.0, np.abs(want)))
    print(f"{kind}: {n} rows, {np.count_nonzero(num)} coupled, worst difference to the union-table product {err:.3e}")
    assert err <= 1e-12
    hij = ham.dense_hij(rd)[:, 0].cpu().numpy() if ham.diag_terms else np.zeros(n)
    assert np.max(np.abs(diag - hij) / np.maximum(1.0, np.abs(hij))) <= 1e-12


# ---- rows that are in the table --------------------------------------------------------------------------------------------
def test_rows_that_are_table_rows(env):
    packed, keys, H, w, v, fci = ref.molecule("H2O")
    S = ref.top_S(H, 200)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, keys[S], ham.device)
    c = np.random.RandomState(9).normal(size=200)
    cd = torch.as_tensor(c, device=ham.device)
    _, num, diag = call(ham, kd, c, -70.0, kd)
    want = ham.matvec(kd, cd).cpu().numpy()
    assert np.max(np.abs(num + diag * c - want) / np.maximum(1.0, np.abs(want))) <= 1e-12
    assert np.allclose(diag, np.diag(H)[S], rtol=0, atol=1e-10 * ref.diag_bound(packed))
    tol = 1e-10
    e0, vec = ham.lowest_eigenpair(kd, tol=tol)
    _, num, diag = call(ham, kd, vec.cpu().numpy(), e0, kd)
    resid = num + diag * vec.cpu().numpy() - e0 * vec.cpu().numpy()
    print(f"residual of the Lanczos vector through naqs_ham_pt2: {np.linalg.norm(resid):.3e} (tolerance {tol * abs(e0):.3e})")
    assert np.linalg.norm(resid) <= 2.0 * tol * max(1.0, abs(e0))


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_arguments(env):
    packed, keys, H, w, v, fci = ref.molecule("LiH")
    lib = env["lib"].load_library()
    ham = env["H"].DevicePauliHamiltonian(packed)
    S = ref.top_S(H, 17)
    kd = dev(env, keys[S], ham.device)
    c = torch.as_tensor(ref.ground(H, S)[1], device=ham.device)
    ext, n_ext = ham.connected_keys(kd)
    num, diag = (torch.empty(n_ext, dtype=torch.float64, device=ham.device) for _ in range(2))
    out4 = torch.full((4,), 7.0, dtype=torch.float64, device=ham.device)
    ok = dict(h=ham._h, M=17, keys=kd.data_ptr(), c=c.data_ptr(), e0=-7.8, n_ext=n_ext, ext=ext.data_ptr(), num=num.data_ptr(),
              diag=diag.data_ptr(), out4=out4.data_ptr(), stream=None)

    def status(**kw):
        a = dict(ok, **kw)
        st = lib.naqs_ham_pt2(a["h"], a["M"], a["keys"], a["c"], ctypes.c_double(a["e0"]), a["n_ext"], a["ext"], a["num"], a["diag"],
                              a["out4"], a["stream"])
        torch.cuda.synchronize()
        return st

    for bad in (dict(h=None), dict(M=0), dict(M=-3), dict(n_ext=-1), dict(keys=None), dict(c=None), dict(out4=None), dict(ext=None),
                dict(e0=float("nan")), dict(e0=float("inf")), dict(e0=float("-inf"))):
        assert status(**bad) == INVALID, bad
    assert status(M=1 << 24) == UNSUPPORTED and status(M=1 << 40) == UNSUPPORTED and status(n_ext=(1 << 30) + 1) == UNSUPPORTED
    assert torch.all(out4 == 7.0)                              # a refused call writes nothing
    assert status(n_ext=0, ext=None) == 0 and torch.all(out4 == 0.0)
    assert status() == 0
    full = (out4.clone(), num.clone(), diag.clone())
    assert full[0][0] < 0 and full[0][2] == 0
    # null num and diag, one at a time and both: the same sums
    for kw in (dict(num=None), dict(diag=None), dict(num=None, diag=None)):
        out4.fill_(7.0)
        assert status(**kw) == 0 and torch.equal(out4, full[0]), kw
    # repetition: the same bits
    for _ in range(3):
        assert status() == 0 and torch.equal(out4, full[0]) and torch.equal(num, full[1]) and torch.equal(diag, full[2])
    # after a larger call (table, rows and the handle's own rows all larger) the small call is a fresh handle's
    big = ref.molecule("LiH")[1]
    big_S = ref.top_S(H, 120)
    bk = dev(env, big[big_S], ham.device)
    bext, bn = ham.connected_keys(bk)
    ham.pt2(bk, torch.ones(120, dtype=torch.float64, device=ham.device), -7.0, bext)
    assert bn > 0 and status(num=None, diag=None) == 0 and torch.equal(out4, full[0])
    assert status() == 0 and torch.equal(num, full[1]) and torch.equal(diag, full[2])
    fresh = env["H"].DevicePauliHamiltonian(packed)
    o2, n2, d2 = fresh.pt2(kd, c, -7.8, ext, rows=True)
    assert torch.equal(o2, full[0]) and torch.equal(n2, full[1]) and torch.equal(d2, full[2])
    with pytest.raises(ValueError):
        ham.pt2(kd, c[:5], -7.8, ext)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_pt2_switch_of_the_command_line(tmp_path, capsys):
    sys.path.insert(0, PKG)
    from experiments import _base
    common = ["-m", os.path.join(GOLDEN, "ham_LiH.npz"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_layer_phase", "2",
              "-n_samps", "100000", "-n_unq_samps_min", "10", "-n_unq_samps_max", "100000", "-n_train", "6", "-output_freq", "2",
              "-lr", "0.001", "-s", "7"]
    res = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "on"), "-pt2"])
    out = capsys.readouterr().out
    summary = open(tmp_path / "on" / "summary.txt").read().splitlines()
    at = [i for i, ln in enumerate(summary) if ln.startswith("sampled-subspace diagonalisation (")]
    assert len(at) == 1
    line = summary[at[0] + 1]
    assert line.startswith("sampled-subspace diagonalisation + Epstein-Nesbet PT2 (") and "connected states) : " in line and "mHa" in line
    assert line in out and "\tpt2 : True" in out
    r = res[0]
    with capsys.disabled():
        print(f"\nLiH after 6 steps: subspace {r['eig']:.8f} ({r['n_unq']} states), E_PT2 {r['e_pt2']:.3e}, FCI {r['fci']:.8f}")
    assert r["e_pt2"] <= 0.0 and abs(r["eig"] + r["e_pt2"] - r["fci"]) <= abs(r["eig"] - r["fci"])
    n_left = [ln for ln in summary if ln.endswith("states at or above the subspace energy left out")]
    assert len(n_left) <= 1
    res = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "off")])
    out = capsys.readouterr().out
    assert "PT2" not in out and "pt2 :" not in out and "PT2" not in open(tmp_path / "off" / "summary.txt").read()
    assert "e_pt2" not in res[0]


def test_solve_h_pt2_draws_what_solve_h_draws(env, tmp_path):
    from test_exact_eloc_gpu import _net, _opt
    hil, wf = _net("LiH", fallback=False)
    opt = _opt("LiH", wf, tmp_path)
    # the state a draw starts from: the generator's, and the wave function's count of sampling calls (its seeds' other half)
    state, calls = opt.generator.get_state(), wf._sample_calls
    eig, vec0, n_unq = opt.solve_H(n_samps=100000)
    after = (opt.generator.get_state(), wf._sample_calls)
    opt.generator.set_state(state)
    wf._sample_calls = calls
    got = opt.solve_H_pt2(n_samps=100000)
    assert torch.equal(opt.generator.get_state(), after[0]) and wf._sample_calls == after[1] == calls + 1
    assert set(got) == {"eig", "vec0", "n_unq", "e_pt2", "n_external", "n_intruders"}
    assert got["eig"] == eig and got["n_unq"] == n_unq and got["vec0"] == pytest.approx(abs(vec0), abs=1e-12)
    fci = float(np.load(os.path.join(GOLDEN, "ham_LiH.npz"))["fci_energy"])
    assert got["e_pt2"] <= 0.0 and got["n_external"] > 0 and abs(eig + got["e_pt2"] - fci) <= abs(eig - fci)
