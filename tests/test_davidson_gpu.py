"""The Davidson solver on the device (``lowest_eigenpair(solver="davidson")``: naqs_ham_eig_lowest) against numpy.linalg.eigh of
the same dense block and against the rule restated in NumPy (tests/davidson_reference.py); tests/test_davidson.py checks on the
CPU that every case here is one the rule converges on within 40 products.

Bounds: |theta - lambda_0| <= 1e-9 Ha (the project's bound for a subspace energy, tests/test_sci_gpu.py: a vector of residual r
errs by r^2 / gap); the dense residual |H x - theta x| <= 2 tol max(1, |theta|) (the rule tests/test_pt2_gpu.py applies to the
Lanczos vector); | |x| - 1 | <= 1e-14; products <= the NumPy rule's count from the same start + 2 (rounding may move the stopping
iteration by one) and <= 40.
"""
import os
import sys

import numpy as np
import pytest

import davidson_reference as dav
import pt2_reference as ref
import sci_reference as sci
from conftest import GOLDEN, PKG
from test_eloc_forms_gpu import naqs_env
from test_eloc_gpu import env  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = dav.T                          # elements a workgroup takes (naqs_eig.hip: EIG_TILE)
TOL = 1e-10


def dev(env, keys, device):
    return env["H"].keys_to_device(np.asarray(keys, np.uint64), device)


def solve(ham, kd, v0=None, **kw):
    if v0 is not None and not torch.is_tensor(v0):
        v0 = torch.as_tensor(np.asarray(v0, np.float64), device=ham.device)
    theta, vec = ham.lowest_eigenpair(kd, solver="davidson", v0=v0, **kw)
    assert ham.last_lanczos_iterations == ham.last_eig_info["products"]
    return theta, vec, dict(ham.last_eig_info)


def held(env, ham, keys, H, lam, seed, tag):
    """One solve from random_start(M, seed) against the dense block: the five checks of the module's docstring."""
    M = len(keys)
    v0 = dav.random_start(M, seed)
    want = dav.davidson(H, v0, tol=TOL)
    theta, vec, info = solve(ham, dev(env, keys, ham.device), v0, tol=TOL)
    x = vec.cpu().numpy()
    resid = np.linalg.norm(H @ x - theta * x)
    print(f"{tag}: M {M}, status {info['status']}, {info['products']} products (NumPy rule {want['products']}), |theta - lambda_0| "
          f"{abs(theta - lam):.2e}, dense residual {resid:.2e}, device residual {info['residual']:.2e}, | |x| - 1 | {abs(np.linalg.norm(x) - 1):.1e}")
    assert info["status"] in (dav.CONVERGED, dav.SPANS), tag
    assert abs(theta - lam) <= 1e-9, tag
    assert resid <= 2.0 * TOL * max(1.0, abs(theta)), tag
    assert abs(np.linalg.norm(x) - 1.0) <= 1e-14, tag
    assert info["products"] <= want["products"] + 2 and info["products"] <= 40, tag
    assert "pt2_kernel<" in ham.last_kernel() and f"eig_gram, ritz, expand, orth x2 <T={T}>" in ham.last_kernel()
    return theta, vec, info


# ---- 1. sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dav.CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_sizes(env, case):
    packed, keys, H, lam = dav.case(*case)
    ham = env["H"].DevicePauliHamiltonian(packed)
    held(env, ham, keys, H, lam, case[2], case)


# ---- 2. both key widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dav.WIDE)
def test_key_widths(env, name):
    packed, keys, H, lam = dav.wide_case(name)
    ham = env["H"].DevicePauliHamiltonian(packed)
    assert ham.key_bits == int(name[-2:])
    held(env, ham, keys, H, lam, 0, name)


# ---- 3. full sectors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_full_sectors(env, mol):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    ham = env["H"].DevicePauliHamiltonian(packed)
    theta, vec, info = held(env, ham, keys, H, float(w[0]), 0, mol)
    assert abs(theta - fci) <= 1e-9
    # the default start is the seeded torch.randn vector the Lanczos path draws
    t_none, v_none, i_none = solve(ham, dev(env, keys, ham.device), tol=TOL)
    gen = torch.Generator(device=ham.device).manual_seed(0)
    start = torch.randn(len(keys), dtype=torch.float64, device=ham.device, generator=gen)
    t_same, v_same, i_same = solve(ham, dev(env, keys, ham.device), start, tol=TOL)
    assert t_none == t_same and torch.equal(v_none, v_same) and i_none == i_same and abs(t_none - fci) <= 1e-9


# ---- 4. the same bits on repetition -----------------------------------------------------------------------------------------------
def same(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_same_bits_on_repetition_and_in_every_form_of_the_walk(env):
    packed, keys, H, lam = dav.case("N2", T + 1, 5)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd, v0 = dev(env, keys, ham.device), dav.random_start(len(keys), 5)
    first = solve(ham, kd, v0, tol=TOL)
    assert same(solve(ham, kd, v0, tol=TOL), first)
    names = {ham.last_kernel()}
    for kw in (dict(STAGE=0), dict(BLOCK=512), dict(BLOOM=1, BLOCK=1024)):
        with naqs_env(**kw):
            assert same(solve(ham, kd, v0, tol=TOL), first), kw
        names.add(ham.last_kernel())
    assert len(names) == 4, names


def test_scratch_regrows_and_the_table_is_rebuilt_per_solve(env):
    packed, keys_l, H_l, lam_l = dav.case("N2", 2 * T + 1, 5)
    _, keys_s, H_s, lam_s = dav.case("N2", T - 1, 5)
    fresh = lambda: env["H"].DevicePauliHamiltonian(packed)          # noqa: E731
    v_l, v_s = dav.random_start(len(keys_l), 5), dav.random_start(len(keys_s), 5)
    ham = fresh()
    kl, ks = dev(env, keys_l, ham.device), dev(env, keys_s, ham.device)
    want_l, want_s = solve(fresh(), kl, v_l, tol=TOL), solve(fresh(), ks, v_s, tol=TOL)
    # small, large (the scratch regrows), small behind large, large again with a wider basis (regrows again), and back
    assert same(solve(ham, ks, v_s, tol=TOL), want_s)
    assert same(solve(ham, kl, v_l, tol=TOL), want_l)
    assert same(solve(ham, ks, v_s, tol=TOL), want_s)
    wide = solve(fresh(), kl, v_l, tol=TOL, m_max=32)
    assert same(solve(ham, kl, v_l, tol=TOL, m_max=32), wide) and abs(wide[0] - lam_l) <= 1e-9
    assert same(solve(ham, kl, v_l, tol=TOL), want_l)
    # other calls on other keys in between: the key table is the solve's own
    other = dev(env, keys_l[::-1][:700].copy(), ham.device)
    ext, n_ext = ham.connected_keys(other)
    ham.pt2(other, torch.ones(700, dtype=torch.float64, device=ham.device), -100.0, ext[:5000])
    assert same(solve(ham, ks, v_s, tol=TOL), want_s)
    ham.local_energy(other, torch.ones((700, 2), dtype=torch.float64, device=ham.device))
    assert same(solve(ham, kl, v_l, tol=TOL), want_l)


# ---- 5. warm starts and statuses --------------------------------------------------------------------------------------------------
def test_warm_start_and_statuses(env):
    packed, fci, k0 = sci.start("N2")
    want = sci.loop(packed, k0, sci.SCHEDULES["N2"])
    ham = env["H"].DevicePauliHamiltonian(packed)
    sizes = [h["M"] for h in want["history"]]
    all_keys = dev(env, want["keys"], ham.device)
    for small, large in list(zip(sizes, sizes[1:]))[-3:]:
        e_small, c, _ = solve(ham, all_keys[:small].contiguous(), tol=TOL)
        kd = all_keys[:large].contiguous()
        e_cold, v_cold, cold = solve(ham, kd, tol=TOL)
        v0 = torch.cat([c, torch.zeros(large - small, dtype=torch.float64, device=ham.device)])
        e_warm, v_warm, warm = solve(ham, kd, v0, tol=TOL)
        print(f"N2 {small} -> {large}: {cold['products']} products cold, {warm['products']} warm")
        assert warm["products"] <= cold["products"] and abs(e_warm - e_cold) <= 1e-9 and e_warm <= e_small + 1e-12
        e_again, v_again, again = solve(ham, kd, v_warm, tol=TOL)
        assert again["products"] == 1 and again["status"] == dav.CONVERGED and abs(e_again - e_warm) <= 1e-12
    e3, v3, i3 = solve(ham, kd, max_iter=3, tol=TOL)
    assert i3["status"] == dav.NOT_CONVERGED and i3["products"] == 3 and np.isfinite(e3) and bool(torch.isfinite(v3).all())
    assert abs(float(v3.norm()) - 1.0) <= 1e-14 and i3["residual"] > TOL * abs(e3) and e3 >= e_cold - 1e-12
    before = dict(ham.last_eig_info)
    for bad in (torch.zeros(large, dtype=torch.float64, device=ham.device),
                torch.full((large,), float("nan"), dtype=torch.float64, device=ham.device),
                torch.ones(large - 1, dtype=torch.float64, device=ham.device)):
        with pytest.raises(ValueError):
            ham.lowest_eigenpair(kd, solver="davidson", v0=bad)
    for kw in (dict(m_max=1), dict(m_max=33), dict(delta=0.0), dict(delta=float("nan")), dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            ham.lowest_eigenpair(kd, solver="davidson", **kw)
    assert ham.last_eig_info == before
    with pytest.raises(ValueError):
        ham.lowest_eigenpair(kd, solver="jacobi")


def test_entry_point_refuses_bad_arguments(env):
    import ctypes
    packed, keys, H, lam = dav.case("LiH", 17, 28)
    ham = env["H"].DevicePauliHamiltonian(packed)
    lib = env["lib"].load_library()
    kd = dev(env, keys, ham.device)
    v0 = torch.ones(17, dtype=torch.float64, device=ham.device)
    vec = torch.full((17,), 7.0, dtype=torch.float64, device=ham.device)
    info = (ctypes.c_double * 4)(9, 9, 9, 9)
    ok = dict(h=ham._h, M=17, keys=kd.data_ptr(), v0=v0.data_ptr(), tol=1e-10, n=400, m=16, delta=1e-2, vec=vec.data_ptr(), info=info)

    def status(**kw):
        a = dict(ok, **kw)
        st = lib.naqs_ham_eig_lowest(a["h"], a["M"], a["keys"], a["v0"], a["tol"], a["n"], a["m"], a["delta"], a["vec"], a["info"], None)
        torch.cuda.synchronize()
        return st

    inf, nan = float("inf"), float("nan")
    for bad in (dict(h=None), dict(M=0), dict(M=-1), dict(keys=None), dict(v0=None), dict(vec=None), dict(info=None), dict(tol=0.0),
                dict(tol=-1e-3), dict(tol=inf), dict(tol=nan), dict(delta=0.0), dict(delta=inf), dict(delta=nan), dict(m=1), dict(m=33),
                dict(n=0), dict(v0=torch.zeros(17, dtype=torch.float64, device=ham.device).data_ptr())):
        assert status(**bad) == -1, bad
    assert status(M=1 << 24) == -4
    assert torch.all(vec == 7.0) and list(info) == [9, 9, 9, 9]             # a refused call writes nothing
    assert status() == 0 and info[3] in (0.0, 2.0) and abs(info[0] - lam) <= 1e-9 and info[2] <= 17


# ---- 6. selected CI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", ["LiH", "H2O", "N2"])
def test_selected_ci_with_the_davidson_solver(env, mol):
    packed, fci, k0 = sci.start(mol)
    want = sci.loop(packed, k0, sci.SCHEDULES[mol])
    ham = env["H"].DevicePauliHamiltonian(packed)
    products = []
    inner = ham.lowest_eigenpair

    def counted(*a, **kw):
        out = inner(*a, **kw)
        assert kw.get("solver") == "davidson"
        products.append(ham.last_eig_info["products"])
        return out

    ham.lowest_eigenpair = counted
    got = ham.selected_ci(dev(env, k0, ham.device), sci.SCHEDULES[mol], tol=1e-13, solver="davidson")
    assert got["stopped"] == want["stopped"] == "schedule" and len(got["history"]) == len(want["history"]) == len(products)
    worst_e = max(abs(g["e0"] - w["e0"]) for g, w in zip(got["history"], want["history"]))
    worst_p = max(abs(g["e_pt2"] - w["e_pt2"]) / abs(w["e_pt2"]) for g, w in zip(got["history"], want["history"]))
    print(f"{mol}: M {[g['M'] for g in got['history']]}, products {products}, worst |E_S - ref| {worst_e:.2e} Ha, "
          f"worst |E_PT2 - ref| / |E_PT2| {worst_p:.2e}")
    for g, w in zip(got["history"], want["history"]):
        assert (g["M"], g["n_external"], g["n_added"]) == (w["M"], w["n_external"], w["n_added"])
        assert abs(g["e0"] - w["e0"]) <= 1e-9
        assert abs(g["e_pt2"] - w["e_pt2"]) <= 1e-8 * abs(w["e_pt2"]) + 1e-13
    assert np.array_equal(got["keys"].cpu().numpy().view(np.uint64), want["keys"])


# ---- 7. the optimiser and the command line ----------------------------------------------------------------------------------------
def test_the_optimiser_with_the_davidson_solver(env, tmp_path):
    from test_exact_eloc_gpu import _net, _opt
    hil, wf = _net("LiH", fallback=False)
    opt = _opt("LiH", wf, tmp_path, eig_solver="davidson")
    state, calls = opt.generator.get_state(), wf._sample_calls

    def rewind():
        opt.generator.set_state(state)
        wf._sample_calls = calls

    eig, vec0, n_unq = opt.solve_H(n_samps=100000)
    assert opt.pauli_hamiltonian.last_eig_info["status"] in (dav.CONVERGED, dav.SPANS)
    rewind()
    opt.eig_solver = "lanczos"
    eig_l, vec0_l, n_unq_l = opt.solve_H(n_samps=100000)
    opt.eig_solver = "davidson"
    assert n_unq == n_unq_l and abs(eig - eig_l) <= 1e-9
    rewind()
    one = opt.solve_H_pt2(n_samps=100000)
    rewind()
    got = opt.solve_H_sci(n_samps=100000, n_iter=3, grow=0.5)
    h0 = got["history"][0]
    assert abs(h0["e0"] - one["eig"]) <= 1e-9 and abs(one["eig"] - eig) <= 1e-9 and h0["n_external"] == one["n_external"]
    assert abs(h0["e_pt2"] - one["e_pt2"]) <= 1e-8 * abs(one["e_pt2"]) + 1e-13
    e = [h["e0"] for h in got["history"]]
    assert all(b <= a + 1e-12 for a, b in zip(e, e[1:]))


def test_eig_solver_switch_of_the_command_line(tmp_path, capsys):
    sys.path.insert(0, PKG)
    from experiments import _base
    common = ["-m", os.path.join(GOLDEN, "ham_LiH.npz"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_layer_phase", "2",
              "-n_samps", "100000", "-n_unq_samps_min", "10", "-n_unq_samps_max", "100000", "-n_train", "6", "-output_freq", "2",
              "-lr", "0.001", "-s", "7", "-pt2"]
    on = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "on"), "-eig_solver", "davidson"])
    out = capsys.readouterr().out
    assert "\teig_solver : davidson" in out
    off = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "off")])
    assert "eig_solver :" not in capsys.readouterr().out and "eig_solver" not in off[0]

    def eig_line(d):
        lines = [ln for ln in open(tmp_path / d / "summary.txt").read().splitlines() if ln.startswith("sampled-subspace diagonalisation (")]
        assert len(lines) == 1
        return float(lines[0].rsplit(":", 1)[1])

    assert abs(on[0]["eig"] - off[0]["eig"]) <= 1e-9 and on[0]["n_unq"] == off[0]["n_unq"]
    assert abs(eig_line("on") - eig_line("off")) <= 1e-8 + 1e-9                   # (the line prints eight decimals)
    assert abs(on[0]["e_pt2"] - off[0]["e_pt2"]) <= 1e-8 * abs(off[0]["e_pt2"]) + 1e-13


# ---- 8. defaults untouched --------------------------------------------------------------------------------------------------------
def test_the_default_is_the_lanczos_path_bit_for_bit(env):
    packed, keys, H, lam = dav.case("LiH", 65, 76)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, keys, ham.device)
    e0, v0 = ham.lowest_eigenpair(kd)
    n0 = ham.last_lanczos_iterations
    assert ham.last_eig_info is None
    e1, v1 = ham.lowest_eigenpair(kd, solver="lanczos")
    assert e0 == e1 and torch.equal(v0, v1) and ham.last_lanczos_iterations == n0 and ham.last_eig_info is None
    assert abs(e0 - lam) <= 1e-9
