"""Closed forms of the E_loc matrix elements (csrc/naqs_closed.hpp) on the CPU: a Python mirror of the
classification and of both closed forms over the four golden Hamiltonians, and the C++ builder (`naqs_closed_group`, which
needs no device) held to the mirror entry for entry.

Bounds.  A class-D element is the loop's sum with every addend negated or not at all: bitwise equal, up to the sign of an
exact zero.  A class-S element is the same n terms in another association: the loop's error and the closed form's are each
<= (n - 1) eps sum|c_t| (sequential sums), so they differ by <= 2 (n - 1) eps sum|c_t|; asserted at that bound, with the
figures printed."""
import ctypes

import numpy as np
import pytest

import closed_reference as cr
from conftest import golden

MOLS = ("LiH", "H2O", "N2", "Li2O")
# non-diagonal groups: (D groups, their terms, S groups, their terms, neither)
EXPECTED = {"LiH": (71, 288, 12, 264, 0), "H2O": (159, 664, 30, 620, 0), "N2": (365, 1572, 12, 456, 0),
            "Li2O": (3745, 16380, 64, 3712, 0)}
EPS = np.finfo(np.float64).eps


def random_keys(n_qubits, n, seed):
    rs = np.random.RandomState(seed)
    keys = [int(rs.randint(0, 1 << 30)) | (int(rs.randint(0, 1 << 30)) << 30) for _ in range(n)]
    full = (1 << n_qubits) - 1
    return [k & full for k in keys] + [0, full, 1 << (n_qubits - 1)]


@pytest.fixture(scope="module", params=MOLS)
def mol(request):
    h = golden(f"ham_{request.param}.npz")
    return request.param, int(h["n_qubits"]), cr.groups(h["xy"], h["yz"], h["coeff"])


def test_class_counts_match_the_table(mol):
    name, _, groups = mol
    nd = ns = td = ts = nl = 0
    for xy, yzs, _ in groups:
        if xy == 0:
            continue
        cls = cr.classify(xy, yzs)[0]
        nd += cls == cr.CLASS_D
        ns += cls == cr.CLASS_S
        nl += cls == cr.CLASS_L
        td += len(yzs) * (cls == cr.CLASS_D)
        ts += len(yzs) * (cls == cr.CLASS_S)
    assert (nd, td, ns, ts, nl) == EXPECTED[name]
    # every D group fits the shortest chunk (8 terms): none falls back to the loop in a handle
    assert max(len(yzs) for xy, yzs, _ in groups if xy and cr.classify(xy, yzs)[0] == cr.CLASS_D) <= 8


def test_d_equals_the_loop_bitwise(mol):
    name, n_qubits, groups = mol
    keys = random_keys(n_qubits, 24, 3)
    step = max(1, len(groups) // 400)                         # Li2O: every ninth group
    checked = 0
    for xy, yzs, cs in groups[::step]:
        cls, R, pos = cr.classify(xy, yzs)
        if cls != cr.CLASS_D:
            continue
        T = cr.build_d(R, pos, yzs, cs)
        for k in keys:
            want, got = cr.loop_element(k, yzs, cs), cr.eval_d(k, R, pos, T)
            assert got == want                                # == : +0.0 and -0.0 compare equal ...
            if want != 0.0:
                assert np.float64(got).tobytes() == np.float64(want).tobytes()
        checked += 1
    assert checked >= 50, name


def test_s_within_the_reassociation_bound(mol):
    name, n_qubits, groups = mol
    keys = random_keys(n_qubits, 24, 5)
    nseg = cr.n_segments(n_qubits)
    worst = 0.0
    s_groups = [(xy, yzs, cs) for xy, yzs, cs in groups if xy and cr.classify(xy, yzs)[0] == cr.CLASS_S]
    for xy, yzs, cs in s_groups[:: max(1, len(s_groups) // 12)]:
        _, R, pos = cr.classify(xy, yzs)
        B = cr.build_s(xy, R, pos, yzs, cs, nseg)
        bound = 2 * (len(cs) - 1) * EPS * sum(abs(c) for c in cs)
        for k in keys:
            d = abs(cr.eval_s(k, R, pos, B) - cr.loop_element(k, yzs, cs))
            worst = max(worst, d / bound)
            assert d <= bound
    print(f"{name}: largest |closed S - loop| = {worst:.3f} of the bound 2 (n - 1) eps sum|c|")


def test_all_patterns_are_filled():
    """Keys outside the particle-number sector (a call without the filter) put every pattern on the flipped positions."""
    h = golden("ham_LiH.npz")
    groups = cr.groups(h["xy"], h["yz"], h["coeff"])
    n_qubits = int(h["n_qubits"])
    for want_cls, n_pat in ((cr.CLASS_D, 16), (cr.CLASS_S, 4)):
        xy, yzs, cs = next(g for g in groups if g[0] and cr.classify(g[0], g[1])[0] == want_cls)
        cls, R, pos = cr.classify(xy, yzs)
        rest = 0b101101110011 & ~xy & ((1 << n_qubits) - 1)
        for p in range(n_pat):
            k = rest | cr.deposit(pos, p)
            assert cr.pattern_of(k, pos) == p
            want = cr.loop_element(k, yzs, cs)
            if cls == cr.CLASS_D:
                assert cr.eval_d(k, R, pos, cr.build_d(R, pos, yzs, cs)) == want
            else:
                got = cr.eval_s(k, R, pos, cr.build_s(xy, R, pos, yzs, cs, cr.n_segments(n_qubits)))
                assert abs(got - want) <= 2 * (len(cs) - 1) * EPS * sum(abs(c) for c in cs)


def test_groups_that_must_fall_back():
    xy4, xy2, xy6 = 0b1111 << 3, 0b101 << 2, 0b111111
    assert cr.classify(xy4, [0b0101 << 3, 0b1111 << 3])[0] == cr.CLASS_D
    assert cr.classify(xy4, [0b0101 << 3, (0b1111 << 3) | 1])[0] == cr.CLASS_L            # one term carries a spectator bit
    assert cr.classify(xy2, [0, 1 << 9, 1 << 11, (1 << 2) | (1 << 12)])[0] == cr.CLASS_S
    assert cr.classify(xy2, [0, 1 << 9, (1 << 11) | (1 << 12) | (1 << 9)])[0] == cr.CLASS_L   # a two-spectator term under every R
    assert cr.classify(xy6, [0, 0b11])[0] == cr.CLASS_L                                   # a 6-bit flip
    # the best R among the group's own terms: under R = yz_0 the third term has two spectators, under R = yz_1 none has
    cls, R, _ = cr.classify(xy2, [1 << 9, (1 << 9) | (1 << 11), (1 << 11)])
    assert cls == cr.CLASS_S and R == (1 << 9) | (1 << 11)


def _native_group(lib, n_qubits, xy, yzs, cs):
    yz = np.asarray(yzs, np.uint64)
    c = np.asarray(cs, np.float64)
    cls, ref = ctypes.c_int32(-1), ctypes.c_uint64(0)
    table = np.full(4 * cr.SEG_SIZE * cr.n_segments(n_qubits), np.nan)
    st = lib.naqs_closed_group(n_qubits, ctypes.c_uint64(xy), len(yz), yz.ctypes.data, c.ctypes.data, ctypes.byref(cls),
                               ctypes.byref(ref), table.ctypes.data)
    assert st == 0
    return cls.value, ref.value, table


def test_native_builder_matches_the_mirror(mol):
    from naqs_amd import _lib
    lib = _lib.load_library()
    name, n_qubits, groups = mol
    nseg = cr.n_segments(n_qubits)
    step = max(1, len(groups) // 150)
    pick = [g for g in groups[::step] if g[0]] + [g for g in groups if g[0] and len(g[1]) > 8][:3]
    seen = set()
    for xy, yzs, cs in pick:
        cls, R, pos = cr.classify(xy, yzs)
        ncls, nref, table = _native_group(lib, n_qubits, xy, yzs, cs)
        assert (ncls, nref) == (cls, R)
        if cls == cr.CLASS_D:
            assert np.array_equal(table[:16], np.array(cr.build_d(R, pos, yzs, cs))) and np.all(np.isnan(table[16:]))
        elif cls == cr.CLASS_S:
            assert np.array_equal(table, cr.build_s(xy, R, pos, yzs, cs, nseg).ravel())
        seen.add(cls)
    assert seen == {cr.CLASS_D, cr.CLASS_S}, name


def test_native_builder_on_fallback_groups():
    from naqs_amd import _lib
    lib = _lib.load_library()
    cls, _, table = _native_group(lib, 20, 0b1111 << 3, [0b0101 << 3, (0b1111 << 3) | 1], [0.5, -0.25])
    assert cls == cr.CLASS_L and np.all(np.isnan(table))
    cls, _, _ = _native_group(lib, 20, 0b111111, [0, 3], [0.5, -0.25])
    assert cls == cr.CLASS_L
    # 64-bit masks: the top bit flipped, a spectator in the last segment
    xy = (1 << 63) | (1 << 5)
    yzs, cs = [1 << 63, (1 << 63) | (1 << 62), 1 << 40], [0.75, -1.5, 0.125]
    cls, ref, table = _native_group(lib, 64, xy, yzs, cs)
    mcls, R, pos = cr.classify(xy, yzs)
    assert cls == mcls == cr.CLASS_S and ref == R and pos == [5, 63]
    assert np.array_equal(table, cr.build_s(xy, R, pos, yzs, cs, cr.n_segments(64)).ravel())
    for k in (0, (1 << 64) - 1, (1 << 63) | (1 << 40), (1 << 62) | (1 << 5)):
        B = table.reshape(cr.n_segments(64), 4, cr.SEG_SIZE)
        assert abs(cr.eval_s(k, R, pos, B) - cr.loop_element(k, yzs, cs)) <= 4 * EPS * sum(abs(c) for c in cs)
