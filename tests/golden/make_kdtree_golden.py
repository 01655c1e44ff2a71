"""Regenerates tests/golden/kdtree_n1024.npz: what the reference's kd-tree builder (PAPC/datasets/tools/build_KDTree.py, build_ClasKDTree)
returns for one synthetic 1024-point cloud.  Needs a checkout of the reference and scipy; only the recorded arrays are committed.

    python tests/golden/make_kdtree_golden.py /path/to/PAPC/datasets/tools/build_KDTree.py

Arrays: cloud [1024, 3] f32 (the input), split_0 .. split_9 int8 (the ten split vectors in the order the builder returns them, lengths
1024, 512, ... 2), leaf_points [1024, 3] f32 (tree[-1][0]: the cloud in the builder's level-0 point order).
"""
import importlib.util
import os
import sys

import numpy as np


def main():
    spec = importlib.util.spec_from_file_location("reference_build_kdtree", sys.argv[1])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(20240521)
    cloud = rng.normal(size=(1024, 3)).astype(np.float32)
    np.random.seed(0)              # (the builder draws only where a leaf holds several identical points: never on this cloud)
    split_dims, tree = mod.build_ClasKDTree(cloud, depth=10)
    assert [len(v) for v in split_dims] == [1024 >> i for i in range(10)] and tree[-1].shape == (1, 1024, 3)
    out = {"cloud": cloud, "leaf_points": np.asarray(tree[-1][0], np.float32)}
    for i, v in enumerate(split_dims):
        out["split_%d" % i] = np.asarray(v).astype(np.int8)
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kdtree_n1024.npz"), **out)


if __name__ == "__main__":
    main()
