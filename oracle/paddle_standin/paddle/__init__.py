"""A stand-in for the ``paddle`` package on torch-CPU -- TEST INFRASTRUCTURE ONLY.

The reference's model code (``PAPC.models.layers``, ``.classify``, ``.segment``) is plain Python over about 45 paddle names.  This package
provides exactly those names, so that the reference's own program text can be imported unmodified and EXECUTED; tests/golden/make_reference_golden.py
does that and commits only the arrays that came out.  What an execution pins is the reference's structure (op order, layouts, concat order,
index quirks, which tensors are parameters, state-dict names).  What it cannot pin is what each Paddle op does: that is ASSUMED here, from
Paddle's documentation, one table entry per behaviour, each held by a hand-computed case in tests/test_paddle_standin.py.

``oracle/paddle_standin`` is never on ``sys.path`` by default: only ``oracle.paddle_standin.on_path()`` puts it there and removes it (and
the modules it loaded) again.  The product and the GPU tests never see it.

Module switches
  ``set_float("float32" | "float64")``  the float type of ``zeros`` / ``ones`` / ``eye``, of ``astype('float32')`` and of new parameters.
                                        float32 is Paddle's own; float64 is used to record values (indices must not depend on it).
  ``TIE_RULE = "all" | "first"``        gradient of ``max`` along an axis among equal maxima (entry T5).
  ``RANDINT_QUEUE``                     list of int64 arrays that ``randint`` pops from (entry T11).
  ``nn.DROPOUT_MASK``                   callable(shape) -> keep mask for ``Dropout`` in train mode (entry L6).

TABLE OF ASSUMED PADDLE BEHAVIOUR (test name in tests/test_paddle_standin.py in brackets)
  T1  to_tensor(ndarray) keeps the numpy dtype (float64 stays float64 in float32 mode), copies, and is a leaf without gradient
      (stop_gradient=True); to_tensor(Tensor) detaches.                                                        [test_to_tensor]
  T2  Tensor.numpy() works on a tensor that carries a graph and returns detached memory.                      [test_numpy_detaches]
  T3  Tensor.astype('float32') / zeros / ones / eye follow the float switch; shapes may be lists or tuples.   [test_float_switch]
  T4  transpose(perm) is a permutation of ALL axes; reshape(shape) accepts -1.                                [test_transpose_reshape]
  T5  max(x, axis[, keepdim]) and Tensor.max return VALUES ONLY.  Gradient: TIE_RULE "all" = every element equal to the maximum receives the
      full gradient (Paddle's documented rule for ``max``, as opposed to ``amax``); "first" = only the first one (what this project's
      kernels do).                                                                                            [test_max_values_and_tie_rule]
  T6  sort(x, axis) and Tensor.sort return VALUES ONLY, ascending, stable.                                    [test_sort_argsort]
  T7  argsort(x, axis) is ascending and stable (equal keys keep their order).                                 [test_sort_argsort]
  T8  argmax(x, axis) returns the FIRST maximal index, int64.                                                 [test_argmax_first]
  T9  sum(x, axis[, keepdim]); matmul batched over leading axes; concat(list, axis); tile(x, repeat_times);
      squeeze(x, axis) of an axis whose size is not 1 is a no-op; index_select(x, index, axis).               [test_small_ops]
  T10 arange -> int64.                                                                                        [test_arange_randint]
  T11 randint(low, high, shape) -> int64; here it pops the next array of RANDINT_QUEUE (the generator queues the farthest-point
      sampling start indices the reference draws there) and checks shape and range.                           [test_arange_randint]
  T12 assigning an integer tensor into a slice of a float tensor casts.                                       [test_setitem_casts]
  L1  nn.Linear: weight [in, out], y = x W + b.                                                               [test_linear]
  L2  nn.BatchNorm1D / 2D / 3D and the fluid-style nn.BatchNorm (any rank, channel axis 1): train mode normalises with the batch mean and
      the BIASED batch variance, eps 1e-5; running = 0.9 * running + 0.1 * batch, the running variance ALSO from the biased batch variance;
      the statistics are named ``_mean`` / ``_variance``, follow ``weight`` / ``bias`` in state_dict(), and are non-trainable;
      eval() normalises with the running values and updates nothing.                                         [test_batchnorm_*]
  L3  nn.Conv1D / 2D / 3D(in, out, kernel, stride=1, padding=0): weight [out, in, *k], cross-correlation, bias [out];
      Conv1DTranspose weight [in, out, k].                                                                    [test_conv]
  L4  nn.ReLU / F.relu; nn.LeakyReLU slope 0.01; nn.LogSoftmax(axis).                                         [test_activations]
  L5  nn.MaxPool1D / 2D / 3D(kernel, stride=None -> kernel, padding=0).                                       [test_maxpool]
  L6  nn.Dropout(p): identity in eval(); in train() x * keep / (1 - p) with keep from nn.DROPOUT_MASK.        [test_dropout]
  L7  nn.Layer registers parameters and sub-layers BY ATTRIBUTE ASSIGNMENT: layers kept in plain Python lists are invisible to
      parameters(), state_dict(), train() and eval().  nn.Sequential names its children '0', '1', ...  state_dict() order: a layer's own
      parameters, then its buffers, then its sub-layers in registration order.                               [test_layer_registration]
  L8  ParamAttr(initializer=Assign(value)) as weight_attr / bias_attr sets the initial value.                 [test_param_attr_assign]

Any other attribute of ``paddle``, ``paddle.nn`` or ``paddle.nn.functional`` raises AttributeError naming it.
"""
import numpy as np
import torch

_FLOAT = torch.float32
TIE_RULE = "all"
RANDINT_QUEUE = []


def set_float(name):
    global _FLOAT
    _FLOAT = {"float32": torch.float32, "float64": torch.float64}[name]


def get_float():
    return _FLOAT


def _dtype(d):
    if isinstance(d, torch.dtype):
        return d
    d = str(d)
    if d in ("float32", "float"):
        return _FLOAT                      # T3
    return {"float64": torch.float64, "int64": torch.int64, "int32": torch.int32, "bool": torch.bool}[d]


def _plain(t):
    return t.as_subclass(torch.Tensor)


def _wrap(t):
    return t.as_subclass(Tensor)


class _MaxAlong(torch.autograd.Function):
    """values of max along one axis (kept); gradient to all maxima or to the first one (T5)"""

    @staticmethod
    def forward(ctx, x, axis, rule):
        m = torch.amax(x, dim=axis, keepdim=True)
        eq = x == m
        if rule == "first":
            eq = eq & (torch.cumsum(eq.to(torch.int64), dim=axis) == 1)
        else:
            assert rule == "all", rule
        ctx.save_for_backward(eq)
        return m

    @staticmethod
    def backward(ctx, g):
        (eq,) = ctx.saved_tensors
        return g * eq.to(g.dtype), None, None


class Tensor(torch.Tensor):
    """torch.Tensor with the paddle spellings the reference uses"""

    def astype(self, d):
        return _wrap(_plain(self).to(_dtype(d)))

    def numpy(self):                                   # T2
        return _plain(self).detach().numpy()

    def transpose(self, perm, *more):                  # T4
        if more:
            perm = (perm,) + more
        perm = list(perm)
        assert sorted(p % self.dim() for p in perm) == list(range(self.dim())), perm
        return _wrap(_plain(self).permute(perm))

    def reshape(self, shape, *more):                   # T4
        if more:
            shape = (shape,) + more
        return _wrap(_plain(self).reshape([int(s) for s in shape]))

    def max(self, axis=None, keepdim=False):           # T5
        return max(self, axis, keepdim)

    def sort(self, axis=-1, descending=False):         # T6
        return sort(self, axis, descending)

    @property
    def stop_gradient(self):
        return not self.requires_grad

    @stop_gradient.setter
    def stop_gradient(self, v):
        self.requires_grad_(not v)


def to_tensor(data, dtype=None, stop_gradient=True):   # T1
    if isinstance(data, torch.Tensor):
        t = _plain(data).detach().clone()
    else:
        a = np.array(data)
        if a.dtype == np.float64 and not isinstance(data, np.ndarray) and not isinstance(data, np.generic):
            a = a.astype({torch.float32: np.float32, torch.float64: np.float64}[_FLOAT])   # python floats: the default float type
        t = torch.from_numpy(a)
    if dtype is not None:
        t = t.to(_dtype(dtype))
    return _wrap(t)


def zeros(shape, dtype=None):
    return _wrap(torch.zeros([int(s) for s in shape], dtype=_FLOAT if dtype is None else _dtype(dtype)))


def ones(shape, dtype=None):
    return _wrap(torch.ones([int(s) for s in shape], dtype=_FLOAT if dtype is None else _dtype(dtype)))


def eye(n, dtype=None):
    return _wrap(torch.eye(int(n), dtype=_FLOAT if dtype is None else _dtype(dtype)))


def arange(start, end=None, step=1):                   # T10
    if end is None:
        start, end = 0, start
    assert all(isinstance(v, (int, np.integer)) for v in (start, end, step)), "only integer ranges are covered"
    return _wrap(torch.arange(int(start), int(end), int(step), dtype=torch.int64))


def randint(low, high, shape):                         # T11
    if not RANDINT_QUEUE:
        raise RuntimeError("paddle.randint: the queue of recorded draws is empty")
    a = np.asarray(RANDINT_QUEUE.pop(0), np.int64)
    assert a.shape == tuple(int(s) for s in shape), (a.shape, shape)
    assert a.min() >= low and a.max() < high, (low, high)
    return _wrap(torch.from_numpy(a.copy()))


def max(x, axis=None, keepdim=False):                  # T5
    assert axis is not None, "only max along one axis is covered"
    m = _MaxAlong.apply(_plain(x), int(axis), TIE_RULE)
    return _wrap(m if keepdim else m.squeeze(int(axis)))


def sum(x, axis=None, keepdim=False):
    assert axis is not None, "only sum along one axis is covered"
    return _wrap(torch.sum(_plain(x), dim=int(axis), keepdim=keepdim))


def sort(x, axis=-1, descending=False):                # T6
    return _wrap(torch.sort(_plain(x), dim=int(axis), descending=descending, stable=True).values)


def argsort(x, axis=-1, descending=False):             # T7
    return _wrap(torch.argsort(_plain(x), dim=int(axis), descending=descending, stable=True))


def argmax(x, axis=None, keepdim=False):               # T8 (numpy documents the first occurrence)
    assert axis is not None and not keepdim
    return _wrap(torch.from_numpy(np.asarray(np.argmax(x.numpy(), axis=int(axis)), np.int64)))


def matmul(x, y):
    return _wrap(torch.matmul(_plain(x), _plain(y)))


def concat(x, axis=0):
    return _wrap(torch.cat([_plain(t) for t in x], dim=int(axis)))


def tile(x, repeat_times):
    r = [int(v) for v in repeat_times]
    assert len(r) == x.dim(), "only full-rank repeat_times are covered"
    return _wrap(_plain(x).repeat(*r))


def reshape(x, shape):
    return x.reshape(list(shape))


def transpose(x, perm):
    return x.transpose(list(perm))


def squeeze(x, axis=None):
    assert axis is not None
    return _wrap(torch.squeeze(_plain(x), dim=int(axis)))     # (a no-op where the axis is longer than 1, as in paddle)


def unsqueeze(x, axis):
    return _wrap(torch.unsqueeze(_plain(x), int(axis)))


def index_select(x, index, axis=0):
    return _wrap(torch.index_select(_plain(x), int(axis), _plain(index).to(torch.int64)))


def summary(*a, **k):
    raise NotImplementedError("paddle.summary is only called under the reference's __main__ guards")


from . import framework, nn                            # noqa: E402  (need Tensor above)

def __getattr__(name):
    raise AttributeError("paddle stand-in: '%s' is not one of the names the reference's model code uses; add it with a table entry and a "
                         "known-answer case" % name)
