"""paddle.nn.functional of the stand-in: relu (table entry L4)."""
import torch

from paddle import _plain, _wrap


def relu(x):
    return _wrap(torch.relu(_plain(x)))


def __getattr__(name):
    raise AttributeError("paddle.nn.functional stand-in: '%s' is not one of the names the reference's model code uses; add it with a table "
                         "entry and a known-answer case" % name)
