"""Exact local energies without a GPU: the numpy restatement of ``naqs_ham_connected``'s definition (used by
tests/test_exact_eloc_gpu.py as the reference), checked against a dense Hamiltonian; the entry point's argument checks;
the ``-exact_eloc`` switch of the command line."""
import ctypes
import sys

import numpy as np
import pytest

from conftest import PKG, dense_pauli_case
from naqs_amd import _lib, packing


def connected_reference(xy, n_qubits, n_alpha, n_beta, keys, row_begin=0, n_rows=None):
    """The definition of include/naqs_hip.h, restated: the keys j = key_i ^ xy_g, i a row of the range, g a non-diagonal
    XY group (xy_g != 0), j passing the particle-number filter (all do for n_alpha = n_beta = -1), j not among ``keys``;
    each once, ascending (uint64)."""
    keys = np.asarray(keys, np.uint64)
    if n_rows is None:
        n_rows = len(keys) - row_begin
    uxy = np.unique(np.asarray(xy, np.uint64))
    uxy = uxy[uxy != 0]
    j = (keys[row_begin:row_begin + n_rows, None] ^ uxy[None, :]).ravel()
    if n_alpha >= 0:
        am = np.uint64(sum(1 << q for q in range(0, n_qubits, 2)))
        bm = np.uint64(sum(1 << q for q in range(1, n_qubits, 2)))
        j = j[(np.bitwise_count(j & am) == n_alpha) & (np.bitwise_count(j & bm) == n_beta)]
    j = np.unique(j)
    return j[~np.isin(j, keys)]


def test_reference_definition_against_a_dense_hamiltonian():
    """6 qubits, no particle filter, random real coefficients (no matrix element of a present group sums to zero): the
    columns outside the table in which the rows' part of the dense matrix is non-zero are exactly the restated set."""
    N = 6
    terms, dense, rs = dense_pauli_case(N)
    ham = packing.pack_qubit_hamiltonian(terms, N, -1, -1)
    for M, (b, n) in ((1, (0, 1)), (7, (0, 7)), (40, (3, 5)), (40, (39, 1)), (40, (0, 40)), (63, (0, 63)), (64, (0, 64)), (40, (5, 0))):
        keys = rs.permutation(1 << N)[:M].astype(np.uint64)
        got = connected_reference(ham.xy, N, -1, -1, keys, b, n)
        rows = keys[b:b + n].astype(int)
        cols = np.nonzero(np.any(dense[rows, :] != 0.0, axis=0))[0].astype(np.uint64) if n else np.zeros(0, np.uint64)
        want = cols[~np.isin(cols, keys)]
        assert np.array_equal(got, want), (M, b, n)
        assert len(np.unique(got)) == len(got)
    assert len(connected_reference(ham.xy, N, -1, -1, np.arange(64, dtype=np.uint64))) == 0


def test_reference_definition_respects_the_particle_filter():
    xy = np.array([0, 0b0101, 0b0011, 0b1111], np.uint64)       # diagonal; alpha hop 0 <-> 2; alpha -> beta; all four flipped
    keys = np.array([0b0011], np.uint64)                        # one alpha (bit 0), one beta (bit 1)
    assert connected_reference(xy, 4, 1, 1, keys).tolist() == [0b0110, 0b1100]
    assert connected_reference(xy, 4, -1, -1, keys).tolist() == [0b0000, 0b0110, 0b1100]


def test_argument_checks_return_invalid_before_any_device_work():
    """Every refusal below is decided from the arguments alone: the handle is never looked into (a buffer of zeros stands
    in for one), so the checks run on a host without a device."""
    lib = _lib.load_library()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake, ctypes.c_void_p)
    keys = np.arange(8, dtype=np.uint64)
    out = np.zeros(8, np.uint64)
    cnt = np.zeros(1, np.int64)
    k, o, c = keys.ctypes.data, out.ctypes.data, cnt.ctypes.data
    f = lib.naqs_ham_connected
    assert f(None, 8, k, 0, 8, 8, o, c, None) == -1          # null handle
    assert f(h, 8, None, 0, 8, 8, o, c, None) == -1          # null keys
    assert f(h, 8, k, 0, 8, 8, o, None, None) == -1          # null count
    assert f(h, -1, k, 0, 0, 8, o, c, None) == -1            # negative sizes
    assert f(h, 8, k, -1, 2, 8, o, c, None) == -1
    assert f(h, 8, k, 0, -2, 8, o, c, None) == -1
    assert f(h, 8, k, 4, 5, 8, o, c, None) == -1             # rows outside [0, M]
    assert f(h, 8, k, 9, 0, 8, o, c, None) == -1
    assert f(h, 8, k, 0, 8, -1, o, c, None) == -1            # capacity < 0
    assert f(h, 8, k, 0, 8, 8, None, c, None) == -1          # nowhere to put capacity > 0 keys
    assert cnt[0] == 0 and not out.any()


def test_binding_and_header_agree_on_the_new_entry_point():
    res, args = _lib.SIGNATURES["naqs_ham_connected"]
    assert res is ctypes.c_int and len(args) == 9
    assert _lib.ABI_VERSION == 9 and _lib.load_library().naqs_abi_version() == 9


def test_parser_accepts_exact_eloc_and_the_reference_command_lines():
    sys.path.insert(0, PKG)
    from experiments._base import get_parser
    p = get_parser(n_hid=128, n_samps=1e7)
    a = p.parse_args("-o data/naqs/N2_s111 -m molecules/N2 -single_phase -n1 -n_layer 1 -n_hid 64 -n_layer_phase 2 "
                     "-n_hid_phase 512 -s 111 -n_train 10000 -output_freq 25 -save_freq -1".split())
    assert a.exact_eloc is False and (a.molecule, a.n_hid, a.n_hid_phase, a.seed) == ("molecules/N2", 64, 512, 111)
    a = p.parse_args("-m molecules/N2_1.5 -full_mask_psi -c -r -v".split())
    assert a.exact_eloc is False and a.full_mask_psi and a.cont and a.resetOpt and a.verbose
    a = p.parse_args("-m molecules/H2O -single_phase -exact_eloc -s 3".split())
    assert a.exact_eloc is True and a.single_phase and a.seed == 3
    with pytest.raises(TypeError):
        get_parser(exact=1)


def test_exact_mode_refuses_the_full_sample_quirk():
    """bug_compat_full_sample_order reorders the table; the exact mode says so before it touches anything."""
    from naqs_amd.optimizer import OptimizerBase
    opt = object.__new__(OptimizerBase)
    opt.bug_compat_full_sample_order = True
    with pytest.raises(NotImplementedError, match="bug_compat_full_sample_order"):
        opt._exact_local_energy(None)
