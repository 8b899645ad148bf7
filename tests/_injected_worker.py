"""Child process of tests/test_gpu_injected_history.py::test_unselected_forms: the first scene with the injected history in a
process of its own, because the two forms it selects are read from the environment once per process
(PLANEVERB_AMD_DECAY_LAUNCHES, PLANEVERB_AMD_SPECTRUM_BLOCK: csrc/pv_solver_maps.cpp).  argv: kind (decay_times | spectrum), the
number of spectrum bins, the .npy to write the kind's whole map to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    kind, nbins, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    from planeverb_amd import api
    import test_gpu_injected_history as inj
    with inj.first_scene(api, nbins) as s:
        s.run(inj.LISTENER)
        inj.adv.inject(s, inj.SEED)
        assert getattr(s, "compute_" + kind)() > 0
        np.save(out, getattr(s, kind)())


if __name__ == "__main__":
    main()
