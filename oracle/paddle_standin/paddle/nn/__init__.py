"""paddle.nn of the stand-in: Layer and the layers the reference's model code constructs (table entries L1 .. L8 of the package docstring)."""
import collections

import numpy as np
import torch
import torch.nn.functional as TF

import paddle
from paddle import Tensor, _plain, _wrap
from . import functional, initializer                         # noqa: F401

DROPOUT_MASK = None          # callable(shape tuple) -> keep mask (array of 0 / 1) for Dropout in train mode (L6)
BN_MOMENTUM = 0.9            # running = momentum * running + (1 - momentum) * batch (L2)
BN_EPSILON = 1e-5


def _param(shape, trainable=True, value=None):
    t = torch.zeros([int(s) for s in shape], dtype=paddle.get_float())
    if value is not None:
        t.copy_(_plain(value).reshape(t.shape))
    t = _wrap(t)
    t.requires_grad_(trainable)
    return t


def _from_attr(attr, shape):
    """a parameter of ``shape``; ParamAttr(initializer=Assign(v)) gives its initial value (L8), anything else zeros (the generator
    overwrites every parameter by its seeded rule)"""
    init = getattr(attr, "initializer", None)
    return _param(shape, value=getattr(init, "value", None))


class Layer:
    """L7: registration by attribute assignment only"""

    def __init__(self, name_scope=None, dtype="float32"):
        d = self.__dict__
        d["_parameters"] = collections.OrderedDict()
        d["_buffers"] = collections.OrderedDict()
        d["_sub_layers"] = collections.OrderedDict()
        d["_pre_hooks"] = []
        d["_post_hooks"] = []
        d["training"] = True

    def __setattr__(self, name, value):
        d = self.__dict__
        if "_parameters" not in d:
            raise RuntimeError("super().__init__() must run before attributes are assigned")
        for reg in (d["_parameters"], d["_buffers"], d["_sub_layers"]):
            reg.pop(name, None)
        if isinstance(value, Layer):
            d["_sub_layers"][name] = value
        elif isinstance(value, Tensor) and getattr(value, "_is_param", False):
            d["_parameters"][name] = value
        else:
            d[name] = value
            return
        d.pop(name, None)

    def __getattr__(self, name):
        d = self.__dict__
        for reg in ("_parameters", "_buffers", "_sub_layers"):
            if reg in d and name in d[reg]:
                return d[reg][name]
        raise AttributeError("%s has no attribute '%s'" % (type(self).__name__, name))

    def create_parameter(self, shape, attr=None, trainable=True):
        p = _from_attr(attr, shape)
        p.requires_grad_(trainable)
        p._is_param = True
        return p

    def register_buffer(self, name, tensor):
        for reg in (self._parameters, self._sub_layers):
            reg.pop(name, None)
        self.__dict__.pop(name, None)
        self._buffers[name] = tensor

    def add_sublayer(self, name, layer):
        self._sub_layers[str(name)] = layer
        return layer

    def named_sublayers(self, prefix="", include_self=False):
        if include_self:
            yield prefix, self
        for n, l in self._sub_layers.items():
            p = prefix + ("." if prefix else "") + n
            yield p, l
            yield from l.named_sublayers(p)

    def sublayers(self, include_self=False):
        return [l for _, l in self.named_sublayers(include_self=include_self)]

    def named_parameters(self, prefix=""):
        for n, p in self._parameters.items():
            yield prefix + ("." if prefix else "") + n, p
        for n, l in self._sub_layers.items():
            yield from l.named_parameters(prefix + ("." if prefix else "") + n)

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def state_dict(self, prefix=""):
        out = collections.OrderedDict()
        dot = prefix + ("." if prefix else "")
        for n, p in self._parameters.items():
            out[dot + n] = p
        for n, b in self._buffers.items():
            out[dot + n] = b
        for n, l in self._sub_layers.items():
            out.update(l.state_dict(dot + n))
        return out

    def train(self):
        self.__dict__["training"] = True
        for l in self._sub_layers.values():
            l.train()

    def eval(self):
        self.__dict__["training"] = False
        for l in self._sub_layers.values():
            l.eval()

    def register_forward_pre_hook(self, hook):
        self._pre_hooks.append(hook)

    def register_forward_post_hook(self, hook):
        self._post_hooks.append(hook)

    def __call__(self, *args, **kwargs):
        for h in self._pre_hooks:
            h(self, args)
        out = self.forward(*args, **kwargs)
        for h in self._post_hooks:
            h(self, args, out)
        return out


class Sequential(Layer):
    def __init__(self, *layers):
        super().__init__()
        for i, l in enumerate(layers):
            self.add_sublayer(str(i), l)

    def __getitem__(self, i):
        return list(self._sub_layers.values())[i]

    def __len__(self):
        return len(self._sub_layers)

    def forward(self, x):
        for l in self._sub_layers.values():
            x = l(x)
        return x


class Linear(Layer):                                          # L1
    def __init__(self, in_features, out_features, weight_attr=None, bias_attr=None):
        super().__init__()
        self.weight = self.create_parameter([in_features, out_features], weight_attr)
        self.bias = self.create_parameter([out_features], bias_attr)

    def forward(self, x):
        return _wrap(torch.matmul(_plain(x), _plain(self.weight)) + _plain(self.bias))


class _ConvNd(Layer):                                         # L3
    ND = 0

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        k = [kernel_size] * self.ND if isinstance(kernel_size, int) else list(kernel_size)
        self._stride, self._padding = stride, padding
        if padding == "same":
            assert all(v == 1 for v in k), "padding='same' is covered for 1-wide kernels only"
            self._padding = 0
        self.weight = self.create_parameter([out_channels, in_channels] + k)
        self.bias = self.create_parameter([out_channels])

    def forward(self, x):
        fn = {1: TF.conv1d, 2: TF.conv2d, 3: TF.conv3d}[self.ND]
        return _wrap(fn(_plain(x), _plain(self.weight), _plain(self.bias), stride=self._stride, padding=self._padding))


class Conv1D(_ConvNd):
    ND = 1


class Conv2D(_ConvNd):
    ND = 2


class Conv3D(_ConvNd):
    ND = 3


class Conv1DTranspose(Layer):                                 # L3
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self._stride, self._padding = stride, padding
        self.weight = self.create_parameter([in_channels, out_channels, kernel_size])
        self.bias = self.create_parameter([out_channels])

    def forward(self, x):
        return _wrap(TF.conv_transpose1d(_plain(x), _plain(self.weight), _plain(self.bias), stride=self._stride, padding=self._padding))


class BatchNorm(Layer):                                       # L2 (the fluid-style layer: any rank, channels on axis 1)
    def __init__(self, num_channels, momentum=BN_MOMENTUM, epsilon=BN_EPSILON):
        super().__init__()
        self._momentum, self._epsilon = momentum, epsilon
        self.weight = self.create_parameter([num_channels])
        self.bias = self.create_parameter([num_channels])
        with torch.no_grad():
            self.weight.fill_(1.0)
        self.register_buffer("_mean", paddle.zeros([num_channels]))
        self.register_buffer("_variance", paddle.ones([num_channels]))

    def forward(self, x):
        x = _plain(x)
        axes = [a for a in range(x.dim()) if a != 1]
        shape = [1, -1] + [1] * (x.dim() - 2)
        if self.training:
            mean = x.mean(dim=axes)
            var = ((x - mean.reshape(shape)) ** 2).mean(dim=axes)                 # biased
            with torch.no_grad():
                m = self._momentum
                _plain(self._mean).mul_(m).add_(mean.detach() * (1.0 - m))
                _plain(self._variance).mul_(m).add_(var.detach() * (1.0 - m))     # ... and the biased one goes into the running value
        else:
            mean, var = _plain(self._mean), _plain(self._variance)
        y = (x - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + self._epsilon)
        return _wrap(y * _plain(self.weight).reshape(shape) + _plain(self.bias).reshape(shape))


class BatchNorm1D(BatchNorm):
    def __init__(self, num_features, momentum=BN_MOMENTUM, epsilon=BN_EPSILON):
        super().__init__(num_features, momentum, epsilon)


class BatchNorm2D(BatchNorm1D):
    pass


class BatchNorm3D(BatchNorm1D):
    pass


class ReLU(Layer):                                            # L4
    def forward(self, x):
        return functional.relu(x)


class LeakyReLU(Layer):
    def __init__(self, negative_slope=0.01):
        super().__init__()
        self._slope = negative_slope

    def forward(self, x):
        x = _plain(x)
        return _wrap(torch.where(x >= 0, x, x * self._slope))


class LogSoftmax(Layer):
    def __init__(self, axis=-1):
        super().__init__()
        self._axis = axis

    def forward(self, x):
        return _wrap(torch.log_softmax(_plain(x), dim=self._axis))


class _MaxPoolNd(Layer):                                      # L5
    ND = 0

    def __init__(self, kernel_size, stride=None, padding=0):
        super().__init__()
        self._k, self._s, self._p = kernel_size, kernel_size if stride is None else stride, padding

    def forward(self, x):
        fn = {1: TF.max_pool1d, 2: TF.max_pool2d, 3: TF.max_pool3d}[self.ND]
        return _wrap(fn(_plain(x), self._k, self._s, self._p))


class MaxPool1D(_MaxPoolNd):
    ND = 1


class MaxPool2D(_MaxPoolNd):
    ND = 2


class MaxPool3D(_MaxPoolNd):
    ND = 3


class Dropout(Layer):                                         # L6
    def __init__(self, p=0.5):
        super().__init__()
        self.p = p

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        if DROPOUT_MASK is None:
            raise RuntimeError("paddle.nn.Dropout in train mode: set paddle.nn.DROPOUT_MASK to a callable(shape) -> keep mask")
        keep = torch.as_tensor(np.asarray(DROPOUT_MASK(tuple(x.shape)))).to(x.dtype)
        return _wrap(_plain(x) * keep / (1.0 - self.p))


def __getattr__(name):
    raise AttributeError("paddle.nn stand-in: '%s' is not one of the names the reference's model code uses; add it with a table entry and a "
                         "known-answer case" % name)
