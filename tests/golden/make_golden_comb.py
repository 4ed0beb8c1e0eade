"""Golden vectors of the single-phase network with combined amplitude-phase blocks (``-single_phase -comb_amp_phase``).

TEST INFRASTRUCTURE — runs only in the build container (needs the reference, like ``make_golden.py``, whose machinery it
reuses unchanged).  The last block's output layer carries the phase rows (nade.py:294-303, 555-560); the constructor makes
the phase symmetry follow the amplitude symmetry, so there are two forms: 5 + 3 outputs with the symmetry, 4 + 4 without.

    python tests/golden/make_golden_comb.py          # comb_LiH_single.npz, comb_LiH_nosym.npz, comb_N2_single.npz

The files are named ``comb_*.npz`` (not ``nade_*.npz``): their content is that of ``make_golden.gen_variant``.
"""
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

mg.VARIANTS.update({
    # -single_phase -comb_amp_phase: no phase MLP; (n_hid_phase, n_layer_phase) are not used by this ansatz
    "comb_single": (dict(combined_amp_phase_blocks=True), (64, 64, 1), mg.NadeMasking.PARTIAL),
    # ... with -no_amp_sym (the phase symmetry follows: 4 + 4 outputs, plain inputs, no sign shift)
    "comb_nosym": (dict(combined_amp_phase_blocks=True, use_amp_spin_sym=False), (64, 64, 1), mg.NadeMasking.PARTIAL),
})

FIXTURES = [("LiH", "comb_single", "comb_LiH_single.npz"),
            ("LiH", "comb_nosym", "comb_LiH_nosym.npz"),
            ("N2", "comb_single", "comb_N2_single.npz")]


def main(which=None):
    tmp = tempfile.mkdtemp(prefix="naqs_comb_golden_")
    try:
        mg.OUT = tmp                                  # gen_variant writes nade_<mol>_<tag>.npz there
        for mol, tag, name in FIXTURES:
            if which and name not in which:
                continue
            mg.gen_variant(mol, tag)
            shutil.move(os.path.join(tmp, f"nade_{mol}_{tag}.npz"), os.path.join(HERE, name))
            print(f"[comb] {name}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1:] or None)
