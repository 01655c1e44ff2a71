"""Regenerates tests/golden/ref_model_vfe_clas.npz and ref_model_vfe_seg.npz: what the REFERENCE'S OWN VFE_Clas() / VFE_Seg() compute when
they are executed on the paddle stand-in (oracle/paddle_standin), recorded by make_reference_golden.run_model on the cloud of ref_layers.npz.
Needs a checkout of the reference; only arrays, names and seeds are committed.

    python tests/golden/make_vfe_golden.py /path/to/reference          (the directory that holds PAPC/)

Running it twice gives byte-identical files.  The contents are those of every ref_model_<name>.npz (see make_reference_golden.py); the
segmenter's per-point tensors (head input [B, 1536, N], logits [B, N, 50]) are stored for every SEG_STRIDE-th point.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_reference_golden import check_recorded, run_model, save_npz   # noqa: E402
from oracle.paddle_standin import on_path                               # noqa: E402


def main():
    ref = os.path.abspath(sys.argv[1])
    lay = np.load(os.path.join(HERE, "ref_layers.npz"))
    planar = np.ascontiguousarray(np.transpose(lay["cloud"], (0, 2, 1)))
    labels = lay["seg_labels"]
    with on_path(ref):
        import paddle
        import paddle.nn as nn
        import PAPC.models.layers.pointnet2_basic_layers as L
        import PAPC.models.classify as C
        import PAPC.models.segment as S
        paddle.TIE_RULE = "all"
        models = {
            "vfe_clas": (lambda: C.VFE_Clas(), planar, "fc", False),
            "vfe_seg": (lambda: S.VFE_Seg(), [planar, labels], "seg_net", True),
        }
        for name, (make, inputs, head, seg) in models.items():
            out, rec = run_model(paddle, nn, L, make, inputs, head, [], seg)
            check_recorded(rec)
            save_npz(os.path.join(HERE, "ref_model_%s.npz" % name), out)


if __name__ == "__main__":
    main()
