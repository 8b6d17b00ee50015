"""Writes tests/golden/cube_increment_parent.npz: what the cube stores' ONE-STORE upkeep -- mml_map_bank_global_increment / _append,
the loop over the banks without `segmented`, and mml_map_global_increment / _append on a context's own store -- returns on a MI355X
for the run functions of tests/test_gpu_bank_cube_segmented.py.  Data only: sizes, centres, and the SHA-256 of every downloaded byte
string and of the association records.

The file in the repository was recorded on the last commit that had a separate one-store chain (k_apply_shifts, k_tag_points, k_hist,
k_classify, k_scatter, k_cube_vox_keys, k_cube_centroid, the match copy through build_grid_into with 32-bit keys) beside the n-store
one, before the two were merged: it is the record of that second implementation, which the merged chain has to reproduce bit for bit
in both call forms and on the own store.  The inputs come from the test module's own run functions and the seeded scene of
conftest.py, so the generator and the tests cannot drift apart.  Needs a GPU and a built library ($MML_LIB_PATH selects another
build).  Rerun: python tests/golden/make_cube_increment_parent.py [out.npz]; two runs give byte-identical files."""
import importlib
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402  (puts the repository root and oracle/ on the path)
import test_gpu_bank_cube_segmented as T  # noqa: E402


def main(path):
    import mml_oracle as O
    O.build()
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    scene = conftest.build_scene(O, synth)
    arrays = {}
    T.digest("history", T._run_history(M, scene, False), arrays)
    T.digest("edge", T._edge_run(M, [0, 1, 2, 3], False), arrays)
    T.digest("move", T._move_run(M, False), arrays)
    T.digest("own", T._own_run(M, scene), arrays)
    T.digest("alone", [T._alone(M, odometry, T._sequence_inputs(synth, w, 7), True) for w in range(3)], arrays)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(arrays[name]), allow_pickle=False)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "entries")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "cube_increment_parent.npz"))
