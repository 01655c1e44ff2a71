"""Shared helpers for the parity tests (oracle = checker; papc_amd = product)."""
import numpy as np


def seeded_weights(chans, seed, bias_scale=0.1):
    """[(conv_w [Cout,Cin], conv_b, gamma, beta)] with non-trivial gamma/beta so BN folding is exercised
    (including NEGATIVE gammas: the max must then pick the smallest pre-BN value)."""
    rng = np.random.default_rng(seed)
    ws = []
    for cin, cout in zip(chans[:-1], chans[1:]):
        w = (rng.normal(size=(cout, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
        b = (rng.normal(size=cout) * bias_scale).astype(np.float32)
        g = rng.uniform(0.5, 1.5, size=cout).astype(np.float32) * rng.choice([1.0, 1.0, 1.0, -1.0], size=cout).astype(np.float32)
        bt = (rng.normal(size=cout) * 0.2).astype(np.float32)
        ws.append((w, b, g, bt))
    return ws


ELEM_FLOOR = 1e-3       # entries at least this fraction of max|ref| are also held elementwise
ELEM_FACTOR = 100.0     # ... to ELEM_FACTOR * rel of THEIR OWN magnitude (default)


def assert_close(got, ref, rel=1e-5, what="", elem=None):
    """Two bars, both asserted.
    (1) max-norm: max|got-ref| <= rel * max|ref| -- the north-star tolerance read on the tensor's scale (activations are O(1) after a BatchNorm,
        and an fp32 accumulation's error is proportional to the magnitude of its terms, not of its result: 1e-5 relative for MLP activations).
    (2) elementwise: every entry with |ref| >= 1e-3 * max|ref| is within ``elem`` of ITS OWN magnitude (default 100 * rel, i.e. 1e-3 at the 1e-5
        bar).  The max-norm bar alone implies only rel / 1e-3 = 1000 * rel there, so this is ten times tighter than what (1) already forces: an
        entry of a thousandth of the tensor's scale may not be off by more than 0.1 % of itself at the 1e-5 bar.  (Round-5 review: a wrong small
        entry hides under a max-norm bar.  Measured on MI355X, round 6: forward comparisons against the float64 oracle sit at 1e-4 .. 5e-4
        elementwise with 3e-7 .. 2e-6 max-norm -- absolute errors are uniform in size, ~1e-6 of the scale, whatever the entry.)
    Callers whose reference legitimately differs in single entries (near-tie routing allowances) state their own ``elem``."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(np.max(np.abs(ref))), 1e-30)
    err = float(np.max(np.abs(got - ref))) / scale
    big = np.abs(ref) >= ELEM_FLOOR * scale
    el = float(np.max(np.abs(got - ref)[big] / np.abs(ref)[big])) if big.any() else 0.0
    ebar = ELEM_FACTOR * rel if elem is None else elem
    print("[assert_close] %s: %.2e of max|ref| (bar %.1e), elementwise %.2e (entries >= 1e-3 max; bar %.1e)" % (what, err, rel, el, ebar))
    assert err <= rel, "%s: max rel err %.3e > %.1e (elementwise %.3e)" % (what, err, rel, el)
    assert el <= ebar, "%s: elementwise rel err %.3e > %.1e on entries >= 1e-3 of max|ref| (max-norm %.3e)" % (what, el, ebar, err)
    return err


def seeded_model_state(model, seed):
    """Deterministic parameter values for a torch module from a numpy generator (independent of torch's RNG streams and of
    the torch version): weights ~ N(0, 2/fan_in), biases ~ 0.1 N(0,1), norm weights in +-[0.5, 1.5], norm biases ~ 0.2 N(0,1).
    Returns {name: float32 ndarray}; copy_into_model() loads it."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, p in model.named_parameters():
        shape = tuple(p.shape)
        if p.dim() >= 2:
            fan_in = int(np.prod(shape[1:]))
            a = rng.normal(size=shape) * np.sqrt(2.0 / fan_in)
        elif "bn" in name or "norm" in name:
            if name.endswith("weight"):
                a = rng.uniform(0.5, 1.5, size=shape) * rng.choice([1.0, 1.0, 1.0, -1.0], size=shape)
            else:
                a = rng.normal(size=shape) * 0.2
        else:
            a = rng.normal(size=shape) * 0.1
        out[name] = a.astype(np.float32)
    return out


def reference_weight(name, shape, seed):
    """The rule (name, shape, seed) -> float32 array behind the tests/golden/ref_*.npz fixtures, which store no weights: the generator gives the
    reference's models these values and the pin tests give them to this project's.  ``name`` / ``shape`` are the REFERENCE's (Linear weights
    [in, out]); layers the reference holds in plain lists are named as this project names them (``sa1.mlp_convs.0.weight``).  Each array has
    its own generator keyed by (seed, CRC-32 of the name), so the values do not depend on the order the names are visited in.
    Matrices / kernels ~ N(0, 2 / fan_in); one-dimensional ``weight`` (only norms have one) in +-[0.5, 1.5] with a quarter negative;
    one-dimensional ``bias`` ~ 0.1 N(0, 1) (0.2 N(0, 1) under a norm would need the layer type: one rule for both)."""
    import zlib
    rng = np.random.default_rng([int(seed), zlib.crc32(name.encode())])
    shape = tuple(int(s) for s in shape)
    if len(shape) >= 2:
        fan_in = shape[0] if len(shape) == 2 else int(np.prod(shape[1:]))
        a = rng.normal(size=shape) * np.sqrt(2.0 / fan_in)
    elif name.endswith("weight"):
        a = rng.uniform(0.5, 1.5, size=shape) * rng.choice([1.0, 1.0, 1.0, -1.0], size=shape)
    else:
        a = rng.normal(size=shape) * 0.1
    return a.astype(np.float32)


def reference_state(names, shapes, seed):
    """{name: reference_weight(...)} for recorded (names, shapes) -- a reference-style state for papc_amd.checkpoint.import_state"""
    return {str(n): reference_weight(str(n), tuple(s[s >= 0]) if isinstance(s, np.ndarray) else s, seed) for n, s in zip(names, shapes)}


def copy_into_model(model, state):
    import torch
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[name]).to(p.device))


def kernel_decisions(out):
    """The decisions the HIP stack behind ``out`` (a shared_mlp_max result that still has its autograd node) took in its forward pass,
    read from the node's saved tensors: (argmax [G, C_L] int32, pooled_alive [G, C_L] bool, masks per non-pooled layer or None).
    A ReLU mask is sign(scale * y + shift) of the kernel's own stored pre-BN output and folded BN constants, evaluated in float64
    (the product of two fp32 numbers is exact there, so the sign is the sign of the kernel's fp32 fma).  Layers whose output the kernel
    never stores (the moment-path first layer, the planes path) return None: their decisions stay the reference's own."""
    fn = out.grad_fn
    for _ in range(4):
        if "MLPMax" in type(fn).__name__ or "MLPStack" in type(fn).__name__:
            break
        fn = fn.next_functions[0][0]
    assert "MLPMax" in type(fn).__name__ or "MLPStack" in type(fn).__name__, type(out.grad_fn).__name__
    saved = fn.saved_tensors
    alive = out.detach() > 0
    if "Planes" in type(fn).__name__:
        return saved[0], alive, None
    L = fn.L
    if "Stack" in type(fn).__name__:       # the library-orchestrated node (papc_amd/stack.py): views into its saved buffer
        from papc_amd.stack import SharedMLPStack
        argmax, ys, consts = SharedMLPStack.views(fn)
    else:
        argmax = saved[5]
        ys, consts = saved[7 + 4 * L: 7 + 5 * L], saved[7 + 5 * L: 7 + 6 * L]
    rowmap = None
    cp = getattr(fn, "compact", None)
    if cp is not None:
        # compacted stack (papc_amd/compact.py): rows are the distinct neighbours; padded slot (g, k) is physical row start[g] + k while k is
        # inside the group's rows and a copy of its first row beyond; argmax holds absolute rows -> offsets in the padded group
        import torch
        start = cp.start.long()
        n = (start[1:] - start[:-1])
        k = torch.arange(cp.K, device=start.device).view(1, -1)
        rowmap = (start[:-1].view(-1, 1) + torch.where(k < n.view(-1, 1), k, torch.zeros_like(k))).reshape(-1)
        argmax = (argmax.long() - start[:-1].view(-1, 1)).to(argmax.dtype)
    masks = []
    for l in range(L - 1):
        y, c = ys[l], consts[l]
        if y is None or y.dim() != 2 or y.shape[1] != c.shape[1]:
            masks.append(None)
        else:
            m = (c[2].double() * y.double() + c[3].double()) > 0
            masks.append(m if rowmap is None else m[rowmap])
    return argmax, alive, masks


def fps_lattice(B, seed, side=26, spacing=0.125):
    """[B, side^3, 3] float32: per cloud its own shuffle of a cubic lattice.  Coordinates are small multiples of 1/8 and every squared distance
    a multiple of 1/64 far below 2^24 / 64, so fp32 computes them EXACTLY in any order: farthest-point sampling on a prefix of such a cloud
    ties among many points in every iteration, and only the first-maximum rule decides (tests/test_oracle.py checks both claims)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(spacing)
    return np.stack([g[rng.permutation(len(g))] for _ in range(B)])
