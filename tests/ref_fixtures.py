"""What the tests of the tests/golden/ref_*.npz fixtures share (tests/test_reference_pin.py on the CPU, tests/test_gpu_reference_pin.py on the
device): loading a fixture, this project's model for a fixture's name, and the seeded weights the generator gave the reference's model
(tests.util.reference_weight over the recorded names and shapes), loaded through papc_amd.checkpoint.import_state."""
import os

import numpy as np

from tests.util import reference_state, reference_weight

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = ("ssg_clas", "msg_clas", "ssg_seg", "basic_clas", "pointnet_clas", "kdnet", "voxnet")
SEG_STRIDE = 32              # the segmenter's per-point tensors are stored for every 32nd point


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def shapes_of(z, key):
    return [tuple(int(v) for v in s[s >= 0]) for s in z[key]]


def sa_weights(prefix, chans, seed):
    ws = []
    for i, (cin, cout) in enumerate(zip(chans[:-1], chans[1:])):
        ws.append((reference_weight("%s.mlp_convs.%d.weight" % (prefix, i), (cout, cin, 1, 1), seed).reshape(cout, cin),
                   reference_weight("%s.mlp_convs.%d.bias" % (prefix, i), (cout,), seed),
                   reference_weight("%s.mlp_bns.%d.weight" % (prefix, i), (cout,), seed),
                   reference_weight("%s.mlp_bns.%d.bias" % (prefix, i), (cout,), seed)))
    return ws


def make_product(name, **kw):
    from papc_amd import models as M
    return {"ssg_clas": lambda: M.PointNet2_SSG_Clas(**kw), "msg_clas": lambda: M.PointNet2_MSG_Clas(**kw), "ssg_seg": lambda: M.PointNet2_SSG_Seg(**kw),
            "basic_clas": M.PointNet_Basic_Clas, "pointnet_clas": lambda: M.PointNet_Clas(max_point=1024), "kdnet": M.KDNet, "voxnet": M.VoxNet}[name]()


def recorded_state(z):
    """a reference-style state for checkpoint.import_state from the fixture's names and shapes: seeded weights, fresh running statistics"""
    names = [str(s) for s in z["state_keys"]] + [str(s) for s in z["list_keys"]]
    shapes = shapes_of(z, "state_shapes") + shapes_of(z, "list_shapes")
    state = reference_state(names, shapes, int(z["weight_seed"]))
    for n, s in zip(names, shapes):
        if n.endswith("._mean"):
            state[n] = np.zeros(s, np.float32)
        elif n.endswith("._variance"):
            state[n] = np.ones(s, np.float32)
    return state, dict(zip(names, shapes))


def seeded_product(name, **kw):
    from papc_amd import checkpoint
    z = gold("ref_model_" + name)
    model = make_product(name, **kw)
    state, _ = recorded_state(z)
    checkpoint.import_state(model, state, strict=True)
    return model, z


