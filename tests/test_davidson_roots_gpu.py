"""The block product (naqs_ham_block_product) and the k-root Davidson solver (``lowest_eigenpairs``: naqs_ham_eig_lowest_k) on the
device: the product bit for bit against naqs_ham_pt2 column by column, the solver against numpy.linalg.eigvalsh of the same
dense block and against the rule restated in NumPy (tests/davidson_roots_reference.py; tests/test_davidson_roots.py checks on
the CPU that every case here is one the rule converges on, and pins its product counts).

Bounds, per root: |theta_j - lambda_j| <= 1e-9 Ha; the dense residual |H x_j - theta_j x_j| <= 2 tol max(1, |theta_j|);
| |x_j| - 1 | <= 1e-14; theta ascending; X X^T - I <= 1e-12; products <= the NumPy rule's count from the same starts + 2 k
(davidson_roots_reference.cap).  Observed on one MI355X: products equal to the rule's in every case; worst |theta - lambda|
2.3e-13 (N2, wide keys), worst dense residual 1.0e-8 against 2.1e-8 allowed (N2, M = 2049, m_max = 16), worst | |x| - 1 | 2.2e-16,
worst X X^T - I 1.3e-15 (LiH, 8 roots).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import davidson_reference as dav
import davidson_roots_reference as R
import pt2_reference as ref
import sci_reference as sci
from conftest import GOLDEN, PKG
from test_eloc_forms_gpu import naqs_env
from test_eloc_gpu import env  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = dav.T
TOL = R.TOL
FORMS = (dict(), dict(STAGE=0), dict(BLOCK=512), dict(BLOOM=1, BLOCK=1024))


def dev(env, keys, device):
    return env["H"].keys_to_device(np.asarray(keys, np.uint64), device)


def on_device(ham, a):
    return torch.as_tensor(np.asarray(a, np.float64), device=ham.device)


# ---- 1. the block product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,seed", [("LiH", 1, 12), ("LiH", 65, 76), ("N2", T + 1, 5)] + [(n, None, 0) for n in dav.WIDE],
                         ids=lambda v: str(v))
def test_block_product_has_the_bits_of_pt2_column_by_column(env, name, M, seed):
    packed, keys, H, w = R.case(name, M, seed)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd, M = dev(env, keys, ham.device), len(keys)
    C = on_device(ham, R.starts(M, 3, 8))
    want = [ham.pt2(kd, C[c], -100.0, kd, rows=True)[1:] for c in range(8)]
    names = set()
    for form in FORMS:
        with naqs_env(**form):
            for nb in range(1, 9):
                num, diag = ham.block_product(kd, C[:nb])
                assert num.shape == (nb, M) and diag.shape == (M,)
                for c in range(nb):
                    assert torch.equal(num[c], want[c][0]) and torch.equal(diag, want[c][1]), (form, nb, c)
                assert f"block_kernel<uint{ham.key_bits}_t, NB={4 if nb <= 4 else 8}, " in ham.last_kernel()
            names.add(ham.last_kernel())
    assert len(names) == (4 if M >= 1024 else 3), names      # (a table below 1 024 rows walks in 512-thread workgroups by default)
    # H C = num + diag C against the dense block (rows of norm ~ sqrt(M), |H| <= ~1e2: a few 1e-12 at most)
    num, diag = ham.block_product(kd, C)
    assert np.abs((num + diag * C).cpu().numpy() - C.cpu().numpy() @ H.T).max() <= 1e-11
    # the padding columns do not leak: a wide run with huge and non-finite columns, then a narrower one on the same handle
    big = C.clone()
    big[2] = 1e300
    big[5] = float("nan")
    ham.block_product(kd, big[:3])
    num2, _ = ham.block_product(kd, big[:2])
    assert torch.equal(num2[0], want[0][0]) and torch.equal(num2[1], want[1][0])
    ham.block_product(kd, big[:6])
    num5, _ = ham.block_product(kd, big[[0, 1, 3, 4, 6]])
    assert all(torch.equal(num5[i], want[c][0]) for i, c in enumerate((0, 1, 3, 4, 6)))
    for bad in (C[:0], torch.cat([C, C[:1]]), C[0], C[:, :-1] if M > 1 else C[:, :0]):
        with pytest.raises(ValueError):
            ham.block_product(kd, bad)


# ---- 2. the solver against the dense block and the rule ---------------------------------------------------------------------------
def solve(ham, kd, k, v0=None, **kw):
    if v0 is not None and not torch.is_tensor(v0):
        v0 = on_device(ham, v0)
    theta, vecs = ham.lowest_eigenpairs(kd, k, v0=v0, **kw)
    assert ham.last_lanczos_iterations == ham.last_eig_info["products"]
    return theta, vecs, dict(ham.last_eig_info)


def held(env, case, count=True):
    name, M, seed, n_roots, m_max = case
    packed, keys, H, w = R.case(name, M, seed)
    ham = env["H"].DevicePauliHamiltonian(packed)
    M = len(keys)
    k = min(n_roots, M)
    theta, vecs, info = solve(ham, dev(env, keys, ham.device), n_roots, R.starts(M, seed, n_roots), tol=TOL, m_max=m_max)
    X = vecs.cpu().numpy()
    resid = np.linalg.norm(X @ H.T - theta[:, None] * X, axis=1)
    norm = np.abs(np.linalg.norm(X, axis=1) - 1.0).max()
    orth = np.abs(X @ X.T - np.eye(k)).max()
    tag = R.case_id(case)
    print(f"{tag}: M {M}, status {info['status']}, {info['products']} products (NumPy rule {R.products(case) if count else '-'}), "
          f"|theta - lambda| {np.abs(theta - w[:k]).max():.2e}, dense residual {resid.max():.2e}, device residual "
          f"{max(info['residuals']):.2e}, | |x| - 1 | {norm:.1e}, X X^T - I {orth:.1e}")
    assert theta.shape == (k,) and tuple(vecs.shape) == (k, M) and len(info["residuals"]) == k, tag
    assert info["status"] in (R.CONVERGED, R.SPANS), tag
    assert np.all(np.abs(theta - w[:k]) <= 1e-9), tag
    assert np.all(resid <= 2.0 * TOL * np.maximum(1.0, np.abs(theta))), tag
    assert norm <= 1e-14 and orth <= 1e-12 and np.all(np.diff(theta) >= 0), tag
    if count:
        assert info["products"] <= R.cap(case), tag
    assert "block_kernel<" in ham.last_kernel() and f"eigk_gram, ritz, expand, settle, orth, accept <T={T}>" in ham.last_kernel()
    return theta, vecs, info


@pytest.mark.parametrize("case", R.SIZES, ids=R.case_id)
def test_sizes(env, case):
    held(env, case)


@pytest.mark.parametrize("case", R.WIDE, ids=R.case_id)
def test_key_widths(env, case):
    held(env, case)


@pytest.mark.parametrize("case", R.SECTORS, ids=R.case_id)
def test_full_sectors(env, case):
    held(env, case)


def test_degenerate_roots(env):
    held(env, R.DEGENERATE, count=False)


@pytest.mark.parametrize("case", R.RESTARTS, ids=R.case_id)
def test_restarts(env, case):
    held(env, case)


def test_the_default_start_is_k_draws_of_the_seeded_generator(env):
    packed, keys, H, w = R.case("LiH*")
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, keys, ham.device)
    none = solve(ham, kd, 3, tol=TOL)
    gen = torch.Generator(device=ham.device).manual_seed(0)
    rows = torch.stack([torch.randn(len(keys), dtype=torch.float64, device=ham.device, generator=gen) for _ in range(3)])
    assert same(solve(ham, kd, 3, rows, tol=TOL), none) and np.all(np.abs(none[0] - w[:3]) <= 1e-9)
    # row 0 is lowest_eigenpair's start
    one, vec = ham.lowest_eigenpair(kd, solver="davidson", tol=TOL)
    again, vec_again = ham.lowest_eigenpair(kd, solver="davidson", tol=TOL, v0=rows[0])
    assert one == again and torch.equal(vec, vec_again)


# ---- 3. one root against naqs_ham_eig_lowest --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dav.CASES + tuple((n, None, 0) for n in dav.WIDE), ids=lambda c: f"{c[0]}-{c[1]}")
def test_one_root_against_the_single_root_solver(env, case):
    packed, keys, H, lam = dav.case(*case)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, keys, ham.device)
    v0 = on_device(ham, dav.random_start(len(keys), case[2]))
    e1, x1 = ham.lowest_eigenpair(kd, solver="davidson", v0=v0, tol=TOL)
    single = dict(ham.last_eig_info)
    theta, vecs, info = solve(ham, kd, 1, v0[None], tol=TOL, m_max=dav.M_MAX)
    print(f"{case}: {info['products']} products both, |d theta| {abs(theta[0] - e1):.1e}, 1 - |x . x'| {1 - abs(float(vecs[0] @ x1)):.1e}")
    assert (info["products"], info["status"]) == (single["products"], single["status"])
    assert abs(theta[0] - e1) <= 1e-12 and abs(float(vecs[0] @ x1)) >= 1.0 - 1e-10


# ---- 4. the same bits -------------------------------------------------------------------------------------------------------------
def same(a, b):
    return np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_same_bits_on_repetition_and_in_every_form_of_the_walk(env):
    packed, keys, H, w = R.case("N2", T + 1, 5)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd, v0 = dev(env, keys, ham.device), R.starts(len(keys), 5, 4)
    first = solve(ham, kd, 4, v0, tol=TOL)
    assert same(solve(ham, kd, 4, v0, tol=TOL), first)
    names = {ham.last_kernel()}
    for form in FORMS[1:]:
        with naqs_env(**form):
            assert same(solve(ham, kd, 4, v0, tol=TOL), first), form
        names.add(ham.last_kernel())
    assert len(names) == 4, names


def test_scratch_regrows_and_the_table_is_rebuilt_per_solve(env):
    packed, keys_l, H_l, w_l = R.case("N2", 2 * T + 1, 5)
    _, keys_s, H_s, w_s = R.case("N2", T - 1, 5)
    fresh = lambda: env["H"].DevicePauliHamiltonian(packed)          # noqa: E731
    v_l, v_s = R.starts(len(keys_l), 5, 4), R.starts(len(keys_s), 5, 4)
    ham = fresh()
    kl, ks = dev(env, keys_l, ham.device), dev(env, keys_s, ham.device)
    want_l, want_s = solve(fresh(), kl, 4, v_l, tol=TOL), solve(fresh(), ks, 4, v_s, tol=TOL)
    want_2 = solve(fresh(), ks, 2, v_s[:2], tol=TOL, m_max=8)
    # small, large (the scratch regrows), small behind large, fewer roots and a narrow basis behind more, and back
    assert same(solve(ham, ks, 4, v_s, tol=TOL), want_s)
    assert same(solve(ham, kl, 4, v_l, tol=TOL), want_l)
    assert same(solve(ham, ks, 4, v_s, tol=TOL), want_s)
    assert same(solve(ham, ks, 2, v_s[:2], tol=TOL, m_max=8), want_2)
    assert same(solve(ham, kl, 4, v_l, tol=TOL), want_l)
    # unrelated calls in between — the single-root solver (the same scratch), a block product and E_loc on other keys
    other = dev(env, keys_l[::-1][:700].copy(), ham.device)
    ham.lowest_eigenpair(other, solver="davidson")
    ham.block_product(other, torch.ones((5, 700), dtype=torch.float64, device=ham.device))
    assert same(solve(ham, ks, 4, v_s, tol=TOL), want_s)
    ham.local_energy(other, torch.ones((700, 2), dtype=torch.float64, device=ham.device))
    assert same(solve(ham, kl, 4, v_l, tol=TOL), want_l)


# ---- 5. statuses and refusals -------------------------------------------------------------------------------------------------------
def test_statuses(env):
    packed, keys, H, w = R.case("N2", T + 1, 5)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd, v0 = dev(env, keys, ham.device), R.starts(len(keys), 5, 4)
    theta, vecs, info = solve(ham, kd, 4, v0, tol=TOL, max_iter=9)
    want = R.davidson_k(H, v0, tol=TOL, max_products=9)
    assert info["status"] == R.NOT_CONVERGED == want["status"] and info["products"] == want["products"] == 12
    assert bool(torch.isfinite(vecs).all()) and np.all(np.abs(vecs.norm(dim=1).cpu().numpy() - 1.0) <= 1e-14)
    assert max(info["residuals"]) > TOL * abs(theta[0]) and np.all(theta >= w[:4] - 1e-12) and np.allclose(theta, want["theta"], atol=1e-9)
    # k = M: the basis spans the space after the start; a tolerance no residual can meet leaves status 2
    packed, keys, H, w = R.case("LiH", 3, 14)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, keys, ham.device)
    for n_roots in (3, 4):
        theta, vecs, info = solve(ham, kd, n_roots, R.starts(3, 14, n_roots), tol=1e-300)
        assert info["status"] == R.SPANS and info["products"] == 3 and np.all(np.abs(theta - w) <= 1e-12) and tuple(vecs.shape) == (3, 3)


def test_refusals(env):
    packed, keys, H, w = R.case("LiH", 17, 28)
    ham = env["H"].DevicePauliHamiltonian(packed)
    lib = env["lib"].load_library()
    kd = dev(env, keys, ham.device)
    v0 = on_device(ham, R.starts(17, 28, 2))
    vecs = torch.full((2, 17), 7.0, dtype=torch.float64, device=ham.device)
    theta, rho, info = (ctypes.c_double * 2)(9, 9), (ctypes.c_double * 2)(9, 9), (ctypes.c_int32 * 2)(9, 9)
    ok = dict(h=ham._h, M=17, keys=kd.data_ptr(), k=2, v0=v0.data_ptr(), tol=1e-10, n=400, m=32, delta=1e-2, vecs=vecs.data_ptr(),
              theta=theta, rho=rho, info=info)

    def status(**kw):
        a = dict(ok, **kw)
        st = lib.naqs_ham_eig_lowest_k(a["h"], a["M"], a["keys"], a["k"], a["v0"], a["tol"], a["n"], a["m"], a["delta"], a["vecs"],
                                       a["theta"], a["rho"], a["info"], None)
        torch.cuda.synchronize()
        return st

    inf, nan = float("inf"), float("nan")
    rows = R.starts(17, 28, 2)
    starts = [np.array([rows[0], rows[0]]), np.array([rows[0], -3.0 * rows[0]]), np.array([rows[0], 0 * rows[0]]),
              np.array([0 * rows[0], rows[1]]), np.array([rows[0], np.full(17, nan)]), np.array([np.full(17, inf), rows[1]])]
    held_starts = [on_device(ham, s) for s in starts]
    for bad in [dict(h=None), dict(M=0), dict(M=-1), dict(keys=None), dict(v0=None), dict(vecs=None), dict(theta=None), dict(rho=None),
                dict(info=None), dict(tol=0.0), dict(tol=-1e-3), dict(tol=inf), dict(tol=nan), dict(delta=0.0), dict(delta=inf),
                dict(delta=nan), dict(k=0), dict(k=9), dict(k=-1), dict(m=3), dict(m=33), dict(k=8, m=15), dict(n=0)] + \
            [dict(v0=s.data_ptr()) for s in held_starts]:
        assert status(**bad) == -1, bad
    assert status(M=1 << 24) == -4
    assert torch.all(vecs == 7.0) and list(theta) == [9, 9] and list(rho) == [9, 9] and list(info) == [9, 9]     # a refused call writes nothing
    assert status() == 0 and info[1] in (0, 2) and np.all(np.abs(np.array(list(theta)) - w[:2]) <= 1e-9) and info[0] <= R.products(("LiH", 17, 28, 2, 32)) + 4
    # the block product's own refusals
    num, diag = torch.empty((2, 17), dtype=torch.float64, device=ham.device), torch.empty(17, dtype=torch.float64, device=ham.device)
    bp = lambda h=ham._h, M=17, k=kd.data_ptr(), nb=2, c=v0.data_ptr(), n=num.data_ptr(), d=diag.data_ptr(): \
        lib.naqs_ham_block_product(h, M, k, nb, c, n, d, None)          # noqa: E731
    assert [bp(h=None), bp(M=0), bp(k=None), bp(nb=0), bp(nb=9), bp(c=None), bp(n=None), bp(d=None)] == [-1] * 8
    assert bp(M=1 << 24) == -4 and bp() == 0
    # the wrapper: a ValueError, and the record of the last solve stays
    before = dict(ham.last_eig_info) if ham.last_eig_info else None
    for s in held_starts:
        with pytest.raises(ValueError):
            ham.lowest_eigenpairs(kd, 2, v0=s)
    with pytest.raises(ValueError):
        ham.lowest_eigenpairs(kd, 2, v0=v0[:1])
    assert ham.last_eig_info == before


# ---- 6. the optimiser and the command line ----------------------------------------------------------------------------------------
def test_solve_h_roots_on_a_trained_network(env, tmp_path):
    from test_exact_eloc_gpu import _net, _opt
    hil, wf = _net("LiH", fallback=False)
    opt = _opt("LiH", wf, tmp_path)
    opt.run(n_epochs=20, save_freq=None, save_final=False, output_freq=10)
    state, calls = opt.generator.get_state(), wf._sample_calls

    def rewind():
        opt.generator.set_state(state)
        wf._sample_calls = calls

    got = opt.solve_H_roots(n_samps=100000, n_roots=3, pt2=True)
    after = (opt.generator.get_state(), wf._sample_calls)
    assert set(got) == {"keys", "eigs", "vec0s", "n_unq", "e_pt2", "n_external", "n_intruders"} and wf._sample_calls == calls + 1      # one draw
    assert opt.pauli_hamiltonian.last_eig_info["status"] in (R.CONVERGED, R.SPANS)
    packed, sector, H, w, v, fci = ref.molecule("LiH")
    keys = got["keys"].cpu().numpy().view(np.uint64)
    assert len(keys) == got["n_unq"] and len(got["eigs"]) == len(got["e_pt2"]) == 3
    lam = np.linalg.eigvalsh(sci.block(packed, keys, keys))
    assert np.all(np.abs(np.array(got["eigs"]) - lam[:3]) <= 1e-9) and got["eigs"] == sorted(got["eigs"])
    # each root's correction against the dense loop over every state outside the sample, with the device's own vector
    S = np.searchsorted(sector, keys)
    assert np.array_equal(sector[S], keys)
    rewind()
    _, vecs = opt.pauli_hamiltonian.lowest_eigenpairs(got["keys"], 3)
    for j in range(3):
        want = ref.pt2(H, S, vecs[j].cpu().numpy(), got["eigs"][j])
        print(f"root {j}: E {got['eigs'][j]:.8f}, E_PT2 {got['e_pt2'][j]:.3e} (dense loop {want['e_pt2']:.3e}), {got['n_external'][j]} connected, "
              f"{got['n_intruders'][j]} intruders")
        assert abs(got["e_pt2"][j] - want["e_pt2"]) < 1e-9 and got["e_pt2"][j] <= 0.0
        assert got["n_external"][j] == got["n_external"][0] > 0
    # root 0 is the ordinary solve_H's state on the same draw; without pt2 the same roots and no correction
    rewind()
    eig, vec0, n_unq = opt.solve_H(n_samps=100000)
    assert torch.equal(opt.generator.get_state(), after[0]) and wf._sample_calls == after[1]
    assert abs(eig - got["eigs"][0]) <= 1e-9 and n_unq == got["n_unq"] and abs(abs(vec0) - got["vec0s"][0]) <= 1e-6
    rewind()
    plain = opt.solve_H_roots(n_samps=100000, n_roots=3)
    assert set(plain) == {"keys", "eigs", "vec0s", "n_unq"} and plain["eigs"] == got["eigs"] and torch.equal(plain["keys"], got["keys"])


def test_roots_switch_of_the_command_line(tmp_path, capsys):
    sys.path.insert(0, PKG)
    from experiments import _base
    common = ["-m", os.path.join(GOLDEN, "ham_LiH.npz"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_layer_phase", "2",
              "-n_samps", "100000", "-n_unq_samps_min", "10", "-n_unq_samps_max", "100000", "-n_train", "6", "-output_freq", "2",
              "-lr", "0.001", "-s", "7", "-pt2"]
    on = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "on"), "-roots", "3"])
    out = capsys.readouterr().out
    assert "\troots : 3" in out
    off = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "off")])
    out_off = capsys.readouterr().out
    assert "\troots :" not in out_off and "sampled-subspace root" not in out_off and "roots" not in off[0]

    def summary(d):
        return [ln for ln in open(tmp_path / d / "summary.txt").read().splitlines() if not ln.startswith("training time")]

    s_on, s_off = summary("on"), summary("off")
    # the roots come last, from a draw of their own: every line of today's summary stands as it is
    assert s_on[:len(s_off)] == s_off and len(s_on) == len(s_off) + 3
    roots = s_on[len(s_off):]
    for j, ln in enumerate(roots):
        assert ln.startswith(f"sampled-subspace root {j} (") and " states) : " in ln and " , gap to root 0 " in ln and " mHa , E + E_PT2 " in ln
        assert ln in out
    e = on[0]["roots"]
    assert len(e) == len(on[0]["roots_e_pt2"]) == 3 and e == sorted(e) and all(p <= 0.0 for p in on[0]["roots_e_pt2"])
    # root 0's line and the diagonalisation's line: the same form, and on this network's draws the same state to the digits printed
    import re
    diag_line = next(ln for ln in s_off if ln.startswith("sampled-subspace diagonalisation ("))
    form = r"^sampled-subspace %s \((\d+) states\) : (-?\d+\.\d{8})"
    m_diag, m_root = re.match(form % "diagonalisation", diag_line), re.match(form % "root 0", roots[0])
    assert m_diag and m_root and abs(float(m_root.group(2)) - e[0]) <= 1e-8 + 1e-9
    # both are variational for the ground state, each on its own draw; the earlier results are the run's without the switch
    fci = on[0]["fci"]
    assert e[0] >= fci - 1e-9 and on[0]["eig"] >= fci - 1e-9 and on[0]["eig"] == off[0]["eig"] and on[0]["e_pt2"] == off[0]["e_pt2"]
