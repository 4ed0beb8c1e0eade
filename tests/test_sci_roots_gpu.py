"""Selected CI for several roots on the device.

* ``naqs_ham_pt2_block``: row c of num, diag and out4[c] against ``naqs_ham_pt2`` with vector c, bit for bit, at every nb that
  meets a compile-time width or its padding, row counts around a wave, a row list that contains table keys, 32- and 64-bit keys,
  more than one workgroup, every form of the walk; the handle's own rows, repetition, padding columns, refusals;
* ``naqs_ham_pt2_select_avg`` against the rule restated in NumPy (tests/sci_roots_reference.py: select), the selected keys and
  both counts array_equal, in both kernel forms; one root of weight 1 against ``naqs_ham_pt2_select``; refusals, overflow;
* the loop ``selected_ci_roots`` against the dense reference loop at the CPU-checked schedules (tests/test_sci_roots.py), with
  the bounds of tests/test_sci_gpu.py: keys equal, |E_j - ref| <= 1e-9 Ha, |E_PT2,j - ref| <= 1e-8 |E_PT2,j| + 1e-13;
* the optimiser and the command line on LiH: iteration 0 is ``solve_H_roots(pt2=True)`` on the same draw, bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

import davidson_roots_reference as D
import pt2_reference as ref
import sci_reference as sci
import sci_roots_reference as R
from conftest import GOLDEN, PKG
from test_eloc_forms_gpu import naqs_env
from test_eloc_gpu import env  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMS = (dict(), dict(STAGE=0), dict(BLOCK=512), dict(BLOOM=1, BLOCK=1024))
WIDTHS = (1, 2, 3, 4, 5, 8)
SELECT_FORMS = {1: "select_one_kernel", 2: "select_hist_kernel x8 + select_count_kernel + select_scan_kernel + select_scatter_kernel"}


def dev(env, keys, device):
    return env["H"].keys_to_device(np.asarray(keys, np.uint64), device)


def host_keys(t):
    return t.cpu().numpy().view(np.uint64)


def on_device(ham, a):
    return torch.as_tensor(np.asarray(a, np.float64), device=ham.device)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the block rows --------------------------------------------------------------------------------------------------------
def singles(ham, kd, C, e, xd):
    """What naqs_ham_pt2 writes for each vector: [(out4, num, diag)]"""
    return [ham.pt2(kd, C[c], float(e[c]), xd, rows=True) for c in range(C.shape[0])]


def same_as_singles(got, want, nb, tag):
    out4, num, diag = got
    assert out4.shape == (nb, 4) and num.shape[0] == nb and num.shape[1] == diag.shape[0]
    for c in range(nb):
        w4, wn, wd = want[c]
        assert torch.equal(num[c], wn) and torch.equal(diag, wd), (tag, c)
        assert np.array_equal(out4[c].cpu().numpy(), w4.cpu().numpy(), equal_nan=True), (tag, c, out4[c], w4)


def test_block_rows_have_the_bits_of_pt2_on_lih(env):
    packed, keys, H, w = D.case("LiH", 17, 28)
    sector = ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    assert len(sector) == 225 and np.all(np.isin(keys, sector))
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, keys, ham.device)
    C = on_device(ham, D.starts(17, 3, 8))
    e = -7.9 + 0.15 * np.arange(8)                   # from below every H_aa to among them: intruders from the third vector on
    n_calls = 0
    for n_ext in (1, 63, 64, 65, 225):
        rows = sector[:n_ext] if n_ext == 225 else sector[100:100 + n_ext]
        xd = dev(env, rows, ham.device)
        want = singles(ham, kd, C, e, xd)
        if n_ext == 225:
            assert sum(int(w4[2]) > 0 for w4, _, _ in want) >= 3 and int(want[0][0][2]) == 0
        for form in FORMS:
            with naqs_env(**form):
                for nb in WIDTHS:
                    got = ham.pt2_block(kd, C[:nb], e[:nb], xd, rows=True)
                    same_as_singles(got, want, nb, (n_ext, form, nb))
                    assert f"block_kernel<uint32_t, NB={4 if nb <= 4 else 8}, " in ham.last_kernel()
                    n_calls += 1
        # the handle's own rows: the same sums, twice, and naqs_ham_pt2's own scratch still stands behind
        for nb in (8, 3, 1):
            for _ in range(2):
                out4 = ham.pt2_block(kd, C[:nb], e[:nb], xd)
                assert all(np.array_equal(out4[c].cpu().numpy(), want[c][0].cpu().numpy(), equal_nan=True) for c in range(nb)), (n_ext, nb)
            assert torch.equal(ham.pt2(kd, C[1], float(e[1]), xd), want[1][0])
    print(f"LiH: {n_calls} block calls equal to naqs_ham_pt2's rows and sums, bit for bit")
    # the padding columns do not leak: a wide call with huge and non-finite vectors, then a narrower one on the same handle
    xd = dev(env, sector, ham.device)
    want = singles(ham, kd, C, e, xd)
    big = C.clone()
    big[2] = 1e300
    big[5] = float("nan")
    ham.pt2_block(kd, big[:6], e[:6], xd, rows=True)
    same_as_singles(ham.pt2_block(kd, big[:2], e[:2], xd, rows=True), want, 2, "narrow behind wide")
    got = ham.pt2_block(kd, big[[0, 1, 3, 4, 6]], e[[0, 1, 3, 4, 6]], xd, rows=True)
    same_as_singles(got, [want[c] for c in (0, 1, 3, 4, 6)], 5, "five of eight")
    # no rows: zeros
    out4, num, diag = ham.pt2_block(kd, C[:3], e[:3], xd[:0], rows=True)
    assert torch.equal(out4, torch.zeros((3, 4), dtype=torch.float64, device=ham.device)) and num.shape == (3, 0) and diag.shape == (0,)


@pytest.mark.parametrize("name,M,seed,nb", [("heavy64", None, 0, 3), ("N2", 2049, 5, 4)], ids=["heavy64-nb3", "N2-2049-nb4"])
def test_block_rows_on_wide_keys_and_many_workgroups(env, name, M, seed, nb):
    packed, keys, H, w = D.case(name, M, seed)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd, M = dev(env, keys, ham.device), len(keys)
    ext, n_ext = ham.connected_keys(kd)
    assert n_ext >= 1024 and ham.key_bits == (64 if name == "heavy64" else 32)      # 1 024-thread workgroups, more than one
    C = on_device(ham, D.starts(M, 7, nb))
    e = float(np.min(np.diag(H))) - 0.5 + 0.4 * np.arange(nb)
    want = singles(ham, kd, C, e, ext)
    names = set()
    for form in FORMS:
        with naqs_env(**form):
            same_as_singles(ham.pt2_block(kd, C, e, ext, rows=True), want, nb, (name, form))
            names.add(ham.last_kernel())
            again = ham.pt2_block(kd, C, e, ext)
            assert all(torch.equal(again[c], want[c][0]) for c in range(nb))
    assert len(names) == 4 and all(f"block_kernel<uint{ham.key_bits}_t, NB=4, " in n for n in names), names
    print(f"{name}: M {M}, {n_ext} external rows, nb {nb}: {sorted(names)}")


def test_block_refusals(env):
    packed, keys, H, w = D.case("LiH", 17, 28)
    ham = env["H"].DevicePauliHamiltonian(packed)
    lib = env["lib"].load_library()
    kd = dev(env, keys, ham.device)
    C = on_device(ham, D.starts(17, 3, 8))
    out4 = torch.full((8, 4), -7.0, dtype=torch.float64, device=ham.device)
    fine = (ctypes.c_double * 8)(*([-8.0] * 8))

    def call(M=17, keys_p=kd.data_ptr(), nb=2, C_p=C.data_ptr(), e=fine, n_ext=17, ext_p=kd.data_ptr(), out_p=out4.data_ptr()):
        return lib.naqs_ham_pt2_block(ham._h, M, keys_p, nb, C_p, e, n_ext, ext_p, None, None, out_p, stream())

    assert call() == 0
    for kw in (dict(nb=0), dict(nb=9), dict(nb=-1), dict(M=0), dict(n_ext=-1), dict(keys_p=None), dict(C_p=None), dict(e=None), dict(ext_p=None),
               dict(out_p=None), dict(e=(ctypes.c_double * 8)(-8.0, float("nan"))), dict(e=(ctypes.c_double * 8)(float("inf"), -8.0))):
        out4.fill_(-7.0)
        assert call(**kw) == -1, kw
        torch.cuda.synchronize()
        assert bool((out4 == -7.0).all()), kw
    assert call(nb=1, e=(ctypes.c_double * 8)(-8.0, float("nan"))) == 0           # only the first nb energies are read
    assert call(M=1 << 24) == -4 and call(n_ext=(1 << 30) + 1) == -4           # NAQS_ERR_UNSUPPORTED
    for bad_C, bad_e in ((C[:0], []), (C[:, :-1], [-8.0] * 8), (C[:2], [-8.0]), (C[:2], [-8.0, float("nan")]), (C[0], [-8.0])):
        with pytest.raises(ValueError):
            ham.pt2_block(kd, bad_C, bad_e, kd)


# ---- 2. the selection ---------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[1, 2])
def form(request):
    with naqs_env(SELECT_FORM=request.param):
        yield request.param


def synthetic(n, nb, seed=0):
    """-> (keys, num [nb, n], diag, e [nb]): every kind of row at once — intruders of one root only and of all, NaNs in one root,
    zeros in one root and in all, infinities, bit-equal ties."""
    rs = np.random.RandomState(1000 * nb + n + seed)
    keys = (rs.permutation(4 * n)[:n].astype(np.uint64) + np.uint64(17)) << np.uint64(3)
    e = -np.arange(nb, dtype=np.float64)                                  # 0, -1, ...: a diag in (-1, 0) is root 0's intruder only
    num = rs.lognormal(size=(nb, n)) * rs.choice([-1.0, 1.0], size=(nb, n))
    diag = rs.lognormal(size=n)
    j = rs.randint(0, 1 << 30, size=n)
    tie = j % 4 == 1
    num[:, tie] = np.round(num[:, tie], 1)
    diag[tie] = 0.5
    kind = rs.randint(0, 20, size=n)
    last = nb - 1
    diag[kind == 0] = -0.5                                                # den < 0 for root 0, > 0 for the others (nb > 1)
    diag[kind == 1] = -(nb + 1.0)                                         # den < 0 for every root
    diag[kind == 2] = 0.0                                                 # den = 0 for root 0
    num[last, kind == 3] = np.nan
    diag[kind == 4] = np.nan
    num[:, kind == 5] = 0.0
    num[0, kind == 6] = -0.0
    num[last, kind == 7] = np.inf
    diag[kind == 8] = np.inf
    num[last, kind == 9] = 0.0
    return keys, num, diag, e


def weights_for(nb, n):
    w = [R.equal_weights(nb), np.random.RandomState(nb + n).uniform(0.1, 2.0, size=nb)]
    if nb > 1:
        z = w[1].copy()
        z[0] = 0.0
        w.append(z)
    return w


def device_select(env, ham, keys, num, diag, e, w, k, **kw):
    sel, n_intr = ham.pt2_select_roots(dev(env, keys, ham.device), on_device(ham, num), on_device(ham, diag), e, k, weights=w, **kw)
    return host_keys(sel), (int(sel.shape[0]), n_intr)


def agree(env, ham, keys, num, diag, e, w, k, **kw):
    got, counts = device_select(env, ham, keys, num, diag, e, w, k, **kw)
    want, want_counts, info = R.select(keys, num, diag, e, R.equal_weights(len(e)) if w is None else w, k, **kw)
    assert counts == want_counts and np.array_equal(got, want), (len(keys), len(e), k, kw, counts, want_counts)
    return info


@pytest.fixture(scope="module")
def ham(env):
    return env["H"].DevicePauliHamiltonian(env["P"].load_packed(os.path.join(GOLDEN, "ham_LiH.npz")))


@pytest.mark.parametrize("nb", [1, 2, 3, 8])
def test_selection_against_the_rule(env, ham, form, nb):
    n_calls = 0
    for n in (1, 255, 256, 257, 2047, 2048, 2049, 4097):
        keys, num, diag, e = synthetic(n, nb)
        for w in weights_for(nb, n):
            eps, intr, elig = R.importance(num, diag, e, w)
            n_el = int(elig.sum())
            s = np.sort(eps[elig])[::-1]
            ks = {0, 1, max(1, n_el // 2), n_el - 1, n_el, n + 5, -2}
            same = np.flatnonzero(s[1:] == s[:-1])
            if len(same):
                ks.add(int(same[len(same) // 2]) + 1)                   # the k-th and the (k+1)-th tie bit for bit
            for k in sorted(ks):
                for rtol in (0.0, 1e-9, 0.5):
                    info = agree(env, ham, keys, num, diag, e, w, k, tie_rtol=rtol)
                    n_calls += 1
                if info["tau"] is not None and np.isfinite(info["tau"]):
                    for eps_min in (float(info["tau"]), float(np.nextafter(info["tau"], np.inf))):
                        agree(env, ham, keys, num, diag, e, w, k, eps_min=eps_min)
                        n_calls += 1
            assert ham.last_kernel() == SELECT_FORMS[form]
        if n == 4097 and nb > 1:
            one_root_only = (diag == -0.5) & ~np.isnan(num).any(axis=0)
            assert one_root_only.sum() > 50 and np.all(np.isinf(R.importance(num, diag, e, R.equal_weights(nb))[0][one_root_only]))
    # weights=None is 1 / nb each
    keys, num, diag, e = synthetic(2049, nb, seed=3)
    got = device_select(env, ham, keys, num, diag, e, None, 300)
    want = R.select(keys, num, diag, e, R.equal_weights(nb), 300)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    print(f"nb {nb} form {form}: {n_calls} calls")


def test_one_live_root_is_the_single_root_call(env, ham, form):
    for n in (257, 4097):
        keys, num, diag, e = synthetic(n, 2)
        kd, nd, dd = dev(env, keys, ham.device), on_device(ham, num), on_device(ham, diag)
        for k in (1, 40, n // 2, n):
            for kw in (dict(), dict(tie_rtol=0.0), dict(eps_min=0.3)):
                one, one_intr = ham.pt2_select(kd, nd[0], dd, float(e[0]), k, **kw)
                for got, got_intr in (ham.pt2_select_roots(kd, nd[:1], dd, e[:1], k, weights=[1.0], **kw),
                                      ham.pt2_select_roots(kd, nd[:1], dd, e[:1], k, **kw),
                                      ham.pt2_select_roots(kd, nd, dd, e, k, weights=[1.0, 0.0], **kw),
                                      ham.pt2_select_roots(kd, nd, dd, [e[0], float("nan")], k, weights=[1.0, 0.0], **kw)):
                    assert torch.equal(got, one) and got_intr == one_intr, (n, k, kw)
                other, other_intr = ham.pt2_select(kd, nd[1], dd, float(e[1]), k, **kw)
                got, got_intr = ham.pt2_select_roots(kd, nd, dd, e, k, weights=[0.0, 1.0], **kw)
                assert torch.equal(got, other) and got_intr == other_intr, (n, k, kw)


def raw_select(env, ham, keys, num, diag, e, w, k, eps_min, rtol, capacity, n_out, nb=None):
    kd = dev(env, keys, ham.device)
    nd, dd = on_device(ham, num), on_device(ham, diag)
    out = torch.full((n_out,), -1, dtype=torch.int64, device=ham.device)
    count = torch.full((2,), -7, dtype=torch.int64, device=ham.device)
    n = len(keys)
    nb = len(e) if nb is None else nb
    st = env["lib"].load_library().naqs_ham_pt2_select_avg(
        ham._h, n, kd.data_ptr() if n else None, nb, nd.data_ptr() if n else None, dd.data_ptr() if n else None,
        (ctypes.c_double * 8)(*e) if e is not None else None, (ctypes.c_double * 8)(*w) if w is not None else None, k, eps_min, rtol,
        capacity, out.data_ptr() if n_out else None, count.data_ptr(), stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), count.cpu().numpy()


def test_selection_overflow_empty_and_refusals(env, ham, form):
    keys, num, diag, e = synthetic(2048 + 77, 3)
    e, w = list(e), [0.5, 0.25, 0.25]
    want, (n_sel, n_intr), _ = R.select(keys, num, diag, e, w, 300)
    assert n_sel >= 300 and n_intr > 0
    st, out, count = raw_select(env, ham, keys, num, diag, e, w, 300, 0.0, 1e-9, n_sel - 1, n_sel + 16)
    assert st == 0 and list(count) == [n_sel, n_intr] and np.all(out[n_sel - 1:] == -1)         # counted, nothing behind the capacity
    st, out, count = raw_select(env, ham, keys, num, diag, e, w, 300, 0.0, 1e-9, 0, 0)
    assert st == 0 and list(count) == [n_sel, n_intr]
    st, out, count = raw_select(env, ham, keys, num, diag, e, w, 300, 0.0, 1e-9, n_sel, n_sel + 16)
    assert st == 0 and list(count) == [n_sel, n_intr] and np.array_equal(out[:n_sel].view(np.uint64), want) and np.all(out[n_sel:] == -1)
    st, out, count = raw_select(env, ham, keys[:0], num[:, :0], diag[:0], e, w, 5, 0.0, 1e-9, 0, 0)
    assert st == 0 and list(count) == [0, 0]
    sel, n_intr0 = ham.pt2_select_roots(dev(env, keys[:0], ham.device), torch.zeros((3, 0)), torch.zeros(0), e, 5)
    assert sel.shape == (0,) and n_intr0 == 0
    nan, inf = float("nan"), float("inf")
    refused = [dict(eps_min=-1.0), dict(rtol=-1e-9), dict(eps_min=nan), dict(rtol=nan), dict(nb=0), dict(nb=9), dict(e=None), dict(w=None),
               dict(w=[0.5, -0.25, 0.25]), dict(w=[0.5, nan, 0.25]), dict(w=[0.5, inf, 0.25]), dict(w=[0.0, 0.0, 0.0]),
               dict(e=[e[0], nan, e[2]]), dict(e=[inf, e[1], e[2]]), dict(capacity=-1)]
    for kw in refused:
        a = dict(e=e, w=w, eps_min=0.0, rtol=0.0, capacity=len(keys), nb=None)
        a.update(kw)
        st, out, count = raw_select(env, ham, keys, num, diag, a["e"] if a["e"] is None else list(a["e"]) + [0.0] * 5,
                                    a["w"] if a["w"] is None else list(a["w"]) + [0.0] * 5, 300, a["eps_min"], a["rtol"], a["capacity"],
                                    len(keys), nb=3 if a["nb"] is None else a["nb"])
        assert st == -1 and list(count) == [-7, -7], kw
    # a root of weight 0 may carry any energy
    st, out, count = raw_select(env, ham, keys, num, diag, [e[0], nan, e[2]], [0.5, 0.0, 0.5], 300, 0.0, 1e-9, len(keys), len(keys))
    want = R.select(keys, num, diag, e, [0.5, 0.0, 0.5], 300)
    assert st == 0 and list(count) == list(want[1]) and np.array_equal(out[:count[0]].view(np.uint64), want[0])
    kd, nd, dd = dev(env, keys, ham.device), on_device(ham, num), on_device(ham, diag)
    for bad in (dict(weights=[0.5, -0.5, 1.0]), dict(weights=[0.0, 0.0, 0.0]), dict(weights=[1.0, 1.0]), dict(weights=[nan, 1.0, 1.0])):
        with pytest.raises(ValueError):
            ham.pt2_select_roots(kd, nd, dd, e, 5, **bad)
    for bad_e in ([e[0], nan, e[2]], e[:2]):
        with pytest.raises(ValueError):
            ham.pt2_select_roots(kd, nd, dd, bad_e, 5)
    with pytest.raises(ValueError):
        ham.pt2_select_roots(kd, nd[0], dd, e[:1], 5)


# ---- 3. the loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", sorted(R.SCHEDULES_ROOTS))
def test_loop_against_the_dense_reference(env, mol):
    n_roots, n_add = R.SCHEDULES_ROOTS[mol]
    packed, fci, k0 = R.start(mol, n_roots)
    want = R.dense_run(mol)
    ham = env["H"].DevicePauliHamiltonian(packed)
    got = ham.selected_ci_roots(dev(env, k0, ham.device), n_roots, n_add, tol=1e-13)
    assert got["stopped"] == want["stopped"] == "schedule" and len(got["history"]) == len(want["history"])
    worst_e = worst_p = 0.0
    for g, w in zip(got["history"], want["history"]):
        assert (g["M"], g["n_external"], g["n_intruders"], g["n_added"]) == (w["M"], w["n_external"], w["n_intruders"], w["n_added"])
        worst_e = max(worst_e, max(abs(a - b) for a, b in zip(g["e0"], w["e0"])))
        worst_p = max(worst_p, max(abs(a - b) / abs(b) for a, b in zip(g["e_pt2"], w["e_pt2"])))
    print(f"{mol} {n_roots} roots: M {[g['M'] for g in got['history']]}, worst |E - ref| {worst_e:.2e} Ha, worst |E_PT2 - ref| / |E_PT2| {worst_p:.2e}")
    assert np.array_equal(host_keys(got["keys"]), want["keys"])
    for g, w in zip(got["history"], want["history"]):
        for j in range(n_roots):
            assert abs(g["e0"][j] - w["e0"][j]) <= 1e-9
            assert abs(g["e_pt2"][j] - w["e_pt2"][j]) <= 1e-8 * abs(w["e_pt2"][j]) + 1e-13
    for a, b in zip(got["history"], got["history"][1:]):
        assert all(y <= x + 1e-12 for x, y in zip(a["e0"], b["e0"]))               # nested subspaces: no root rises
    V = got["vecs"]
    assert V.shape == (n_roots, want["history"][-1]["M"]) and got["eigs"] == got["history"][-1]["e0"]
    assert float((V @ V.T - torch.eye(n_roots, dtype=torch.float64, device=V.device)).abs().max()) <= 1e-12
    for j in range(n_roots):
        series = [dict(e0=h["e0"][j], e_pt2=h["e_pt2"][j]) for h in want["history"]]
        assert got["extrapolated"][j] == pytest.approx(env["H"].extrapolate_pt2(series), abs=1e-7)


def test_loop_early_stops_and_the_closed_sector(env):
    packed, fci, k0 = R.start("LiH", 3)
    ham = env["H"].DevicePauliHamiltonian(packed)
    kd = dev(env, k0, ham.device)
    res = ham.selected_ci_roots(kd, 3, (1000,) * 8, tol=1e-13)
    last = res["history"][-1]
    lam = ref.molecule("LiH")[3]
    assert res["stopped"] == "connected set empty" and last["n_external"] == 0 and last["M"] == 69 and last["e_pt2"] == [0.0] * 3
    assert np.all(np.abs(np.array(res["eigs"]) - lam[:3]) <= 1e-9) and abs(res["eigs"][0] - fci) <= 1e-9
    res = ham.selected_ci_roots(kd, 3, (3, 6, 12, 24), max_states=20)
    assert res["stopped"] == "max_states" and [h["M"] for h in res["history"]] == [3, 6, 13] and res["keys"].shape[0] == 13
    res = ham.selected_ci_roots(kd, 3, (3, 6), eps_min=1e3)
    assert res["stopped"] == "nothing eligible" and len(res["history"]) == 1 and res["extrapolated"] == [None] * 3
    res = ham.selected_ci_roots(kd, 3, (3, 1.0))
    assert [h["M"] for h in res["history"]] == [3, 6, 13] and res["stopped"] == "schedule"
    # a root of weight 0 does not steer the growth: the ground state's own selection, three roots still solved
    res = ham.selected_ci_roots(kd, 3, (3, 6), weights=[1.0, 0.0, 0.0], tol=1e-13)
    want = R.loop(packed, k0, 3, (3, 6), weights=[1.0, 0.0, 0.0])
    assert np.array_equal(host_keys(res["keys"]), want["keys"]) and len(res["eigs"]) == 3
    with pytest.raises(ValueError):
        ham.selected_ci_roots(kd[:2], 3, (3, 6))
    with pytest.raises(ValueError, match="max_external"):
        ham.selected_ci_roots(kd, 3, (3, 6), max_external=10)


# ---- 4. the optimiser and the command line ------------------------------------------------------------------------------------
def test_solve_h_roots_sci_starts_where_solve_h_roots_stands(env, tmp_path):
    from test_exact_eloc_gpu import _net, _opt
    hil, wf = _net("LiH", fallback=False)
    opt = _opt("LiH", wf, tmp_path)
    opt.run(n_epochs=20, save_freq=None, save_final=False, output_freq=10)
    state, calls = opt.generator.get_state(), wf._sample_calls

    def rewind():
        opt.generator.set_state(state)
        wf._sample_calls = calls

    one = opt.solve_H_roots(n_samps=100000, n_roots=3, pt2=True)
    after = (opt.generator.get_state(), wf._sample_calls)
    rewind()
    got = opt.solve_H_roots_sci(n_samps=100000, n_roots=3, n_iter=3, grow=0.5)
    assert torch.equal(opt.generator.get_state(), after[0]) and wf._sample_calls == after[1] == calls + 1            # one draw
    h0 = got["history"][0]
    assert (h0["e0"], h0["e_pt2"], [h0["n_external"]] * 3, h0["n_intruders"], got["n_unq"]) == \
        (one["eigs"], one["e_pt2"], one["n_external"], one["n_intruders"], one["n_unq"])                         # bit for bit
    assert h0["M"] == one["keys"].shape[0] and torch.equal(got["keys"][:h0["M"]], one["keys"])
    hist = got["history"]
    for a, b in zip(hist, hist[1:]):
        assert all(y <= x + 1e-12 for x, y in zip(a["e0"], b["e0"]))
    assert got["stopped"] in ("schedule", "connected set empty", "nothing eligible") and (len(hist) == 3) == (got["stopped"] == "schedule")
    keys = host_keys(got["keys"])
    lam = np.linalg.eigvalsh(sci.block(ref.molecule("LiH")[0], keys, keys))
    assert np.all(np.abs(np.array(got["eigs"]) - lam[:3]) <= 1e-9)
    print(f"LiH after 20 steps: M {[h['M'] for h in hist]}, roots {[[round(x, 6) for x in h['e0']] for h in hist]}")
    rewind()
    cut = opt.solve_H_roots_sci(n_samps=100000, n_roots=3, n_iter=2, n_start=1)
    assert cut["history"][0]["M"] == 3 and cut["n_unq"] == one["n_unq"]                       # n_start is raised to n_roots
    rewind()
    cut = opt.solve_H_roots_sci(n_samps=100000, n_roots=2, n_iter=2, n_start=7)
    assert cut["history"][0]["M"] == 7 and len(cut["eigs"]) == 2 and cut["history"][1]["M"] >= 14


def test_sci_roots_switch_of_the_command_line(tmp_path, capsys):
    sys.path.insert(0, PKG)
    from experiments import _base
    common = ["-m", os.path.join(GOLDEN, "ham_LiH.npz"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_layer_phase", "2",
              "-n_samps", "100000", "-n_unq_samps_min", "10", "-n_unq_samps_max", "100000", "-n_train", "6", "-output_freq", "2",
              "-lr", "0.001", "-s", "7", "-pt2", "-roots", "3", "-sci", "3"]
    on = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "on"), "-sci_roots"])
    out = capsys.readouterr().out
    assert "\tsci_roots : True" in out
    off = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "off")])
    out_off = capsys.readouterr().out
    assert "\tsci_roots" not in out_off and "selected CI for" not in out_off and not any(k.startswith("roots_sci") for k in off[0])

    def summary(d):
        return [ln for ln in open(tmp_path / d / "summary.txt").read().splitlines() if not ln.startswith("training time")]

    s_on, s_off = summary("on"), summary("off")
    new = s_on[len(s_off):]
    hist = on[0]["roots_sci_history"]
    # iteration 0 of the roots' stage is solve_H_roots(pt2=True) on the same draw, bit for bit: every line of the run without the
    # switch stands as it is, the roots' own three among them, and the growth's lines follow
    assert s_on[:len(s_off)] == s_off and sum(ln.startswith("sampled-subspace root ") for ln in s_off) == 3
    assert len(new) == len(hist) + 3 + 1 and all(ln in out for ln in new)
    for t, h in enumerate(hist):
        assert new[t].startswith(f"selected CI for 3 roots iteration {t} ({h['M']} states, {h['n_external']} connected) : E ")
        assert new[t].endswith(" , ".join(f"{e:.8f}" for e in h["e0"]))
    for j in range(3):
        ln = new[len(hist) + j]
        assert ln.startswith(f"selected CI root {j} ({hist[-1]['M']} states) : {on[0]['roots_sci_eigs'][j]:.8f} , gap to root 0 ")
        assert " mHa , E + E_PT2 " in ln and " , extrapolated to E_PT2 = 0 (non-variational) " in ln
    assert new[-1] == f"selected CI for 3 roots stopped : {on[0]['roots_sci_stopped']}"
    assert on[0]["roots"] == hist[0]["e0"] == off[0]["roots"] and on[0]["roots_e_pt2"] == hist[0]["e_pt2"] == off[0]["roots_e_pt2"]
    e = on[0]["roots_sci_eigs"]
    assert e == sorted(e) and all(b <= a + 1e-12 for a, b in zip(hist[0]["e0"], e)) and e[0] >= on[0]["fci"] - 1e-9
    # everything before the roots' stage is the run's without the switch
    assert on[0]["eig"] == off[0]["eig"] and on[0]["e_pt2"] == off[0]["e_pt2"] and on[0]["sci_history"] == off[0]["sci_history"]
