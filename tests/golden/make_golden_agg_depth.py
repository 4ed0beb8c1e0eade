"""Golden vectors of the aggregate-phase network with two hidden layers in every block (run.py's default ansatz with ``-n_layer 2``).

TEST INFRASTRUCTURE — runs only in the build container (needs the reference, like ``make_golden.py``, whose machinery it
reuses unchanged).  ``-n_layer 2`` gives the amplitude blocks two hidden layers, and ``-n_layer_phase`` / ``-n_hid_phase``
follow ``-n_layer`` / ``-n_hid`` (experiments/_base.py), so every per-pair phase block has two hidden layers of the same width.
The width is 32 (16 on N2) rather than run.py's 128 to keep the files small; the kernels' widths are covered by
tests/test_agg_depth_gpu.py.

    python tests/golden/make_golden_agg_depth.py     # aggdepth_LiH.npz, aggdepth_LiH_phasesym.npz, aggdepth_N2.npz

The files are named ``aggdepth_*.npz`` (not ``nade_*.npz``): their content is that of ``make_golden.gen_variant``.
"""
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

N_HID = 32
mg.VARIANTS.update({
    # run.py's default ansatz with -n_layer 2: amplitude and per-pair phase blocks of two hidden layers
    "aggdepth": (dict(aggregate_phase=True, amp_hidden_size=[N_HID] * 2), (N_HID, N_HID, 2), mg.NadeMasking.PARTIAL),
    # ... with -phase_sym (spin-ordered inputs of every phase block, 3 outputs, the sign shift on the last block)
    "aggdepth_phasesym": (dict(aggregate_phase=True, use_phase_spin_sym=True, amp_hidden_size=[N_HID] * 2), (N_HID, N_HID, 2),
                          mg.NadeMasking.PARTIAL),
    # N2 (10 pairs): 16 units, the narrowest width of the family
    "aggdepth16": (dict(aggregate_phase=True, amp_hidden_size=[16] * 2), (16, 16, 2), mg.NadeMasking.PARTIAL),
})

_nade_vectors = mg.nade_vectors


def _small_vectors(wf, opt, hil, all_keys, n_draw=None):
    """make_golden.nade_vectors with a draw of 2 * 10^4 samples on the large spaces (10^3 - 2 * 10^3 unique states, not ~10^4)
    and without the per-pair conditionals, which the tests of this ansatz do not read: the files stay small."""
    nd = _nade_vectors(wf, opt, hil, all_keys, n_draw=n_draw if n_draw is not None or len(all_keys) < 1000 else 20000)
    nd.pop("eval_cond", None)
    return nd


mg.nade_vectors = _small_vectors

FIXTURES = [("LiH", "aggdepth", "aggdepth_LiH.npz"),
            ("LiH", "aggdepth_phasesym", "aggdepth_LiH_phasesym.npz"),
            ("N2", "aggdepth16", "aggdepth_N2.npz")]


def main(which=None):
    tmp = tempfile.mkdtemp(prefix="naqs_aggdepth_golden_")
    try:
        mg.OUT = tmp                                  # gen_variant writes nade_<mol>_<tag>.npz there
        for mol, tag, name in FIXTURES:
            if which and name not in which:
                continue
            mg.gen_variant(mol, tag)
            shutil.move(os.path.join(tmp, f"nade_{mol}_{tag}.npz"), os.path.join(HERE, name))
            print(f"[aggdepth] {name}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:] or None)
