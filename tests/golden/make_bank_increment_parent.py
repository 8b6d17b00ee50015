"""Writes tests/golden/bank_increment_parent.npz: what mml_map_bank_increment -- the loop over the banks, without `segmented` --
returns on a MI355X for the inputs of tests 1-4 and 6 of tests/test_gpu_bank_increment_segmented.py.  Data only: sizes, poses, and
the SHA-256 of every downloaded byte string (bank_download clouds, factor records and their source indices).

The file in the repository was recorded on the last commit that had a separate single-map increment chain (k_to_world, k_concat,
k_vox_keys, k_vox_centroid, build_grid_into's own kernels) beside the segmented one, before the two were merged: it is the record of
that second implementation, which the merged chain has to reproduce bit for bit in both call forms.  The inputs come from the test
module's own run_* functions and the seeded scene of conftest.py, so the generator and the tests cannot drift apart.  Needs a GPU and
a built library ($MML_LIB_PATH selects another build).  Rerun: python tests/golden/make_bank_increment_parent.py [out.npz]; two runs
give byte-identical files."""
import importlib
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402  (puts the repository root and oracle/ on the path)
import test_gpu_bank_increment_segmented as T  # noqa: E402


def main(path):
    import mml_oracle as O
    O.build()
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    scene = conftest.build_scene(O, synth)
    arrays = {}
    for run in (T.run_histories(M, scene, synth, False), T.run_ring_wrap(M, scene, synth, False), T.run_refinement(M, False),
                T.run_batch_odometry(M, synth, "loop")):
        arrays.update(T.digest(run))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(arrays[name]), allow_pickle=False)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "entries")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "bank_increment_parent.npz"))
