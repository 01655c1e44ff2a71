"""ShapeNet-part batch loaders with the reference's semantics (PAPC/datasets/pnloader.py:7-106, dataloader.py:5-40,
file lists datalist.py:1-3) -- the data format on the input side of the hot path.

What the reference does, and what is kept:

* every file of the split is read whole and concatenated in list order: ``f['data'][:, :max_point, :]`` (the FIRST max_point points of each
  cloud, no resampling), ``f['label']`` ([n, 1]), for segmentation also ``f['pid'][:, :max_point]`` (pnloader.py:13-31, 60-81);
* the loader is a generator FACTORY: calling the returned function starts one epoch (pnloader.py:37-50, 89-104);
* ``mode == 'train'`` shuffles the sample order in place with the global ``random`` module at the start of every epoch -- the permutation is
  applied to the previous epoch's order, not to 0..n-1 (pnloader.py:35-39) -- so ``random.seed(s)`` reproduces the reference's batches;
* a batch is ``(data [b, 3, max_point] float32, label [b, 1] int64)`` -- each cloud transposed to channels-first (pnloader.py:43-46) --, for
  segmentation ``([data, label], target [b, max_point, 1] int64)`` (pnloader.py:96-100); the last batch of an epoch may be short
  (pnloader.py:49-50, 103-104).

What is done differently (same batches, bit for bit -- tests/test_datasets.py holds them to a literal restatement, oracle/loaders_ref.py):
the clouds are transposed and converted ONCE at load time into one contiguous ``[n, 3, max_point]`` float32 array (the reference transposes
and converts every sample of every epoch and builds each batch from a Python list), and a batch is one gather along the shuffled order.

Files: ``h5py`` is not part of this image.  ``opener(path)`` returns any mapping with ``['data']`` / ``['label']`` / ``['pid']`` arrays; the
default opener takes ``.h5`` through h5py when it is importable and otherwise (or for ``.npz``) reads a numpy archive with the same keys at
the same stem, so a ShapeNet-part directory converted with ``convert_h5_to_npz`` (on a machine that has h5py) trains here unchanged.
"""
import os
import random

import numpy as np

# PAPC/datasets/datalist.py:1-3
train_list = ['ply_data_train0.h5', 'ply_data_train1.h5', 'ply_data_train2.h5', 'ply_data_train3.h5', 'ply_data_train4.h5', 'ply_data_train5.h5']
test_list = ['ply_data_test0.h5', 'ply_data_test1.h5']
val_list = ['ply_data_val0.h5']


def default_opener(path):
    """``path`` (an .h5 name from the file lists) -> mapping of arrays.  h5py when available, else the .npz twin of the file."""
    stem, ext = os.path.splitext(path)
    if ext == ".h5" and os.path.exists(path):
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(path, "r") as f:
                return {k: np.asarray(f[k]) for k in f.keys()}
    for cand in (path, stem + ".npz"):
        if cand.endswith(".npz") and os.path.exists(cand):
            with np.load(cand) as z:
                return {k: z[k] for k in z.files}
    raise FileNotFoundError("%s: no readable file (h5py %s; looked for %s.npz too)" %
                            (path, "missing" if ext == ".h5" else "not needed", stem))


def convert_h5_to_npz(src_dir, dst_dir=None):
    """One-off helper for a machine with h5py: write the .npz twin of every file of the three lists."""
    import h5py
    dst_dir = dst_dir or src_dir
    for name in train_list + test_list + val_list:
        p = os.path.join(src_dir, name)
        if os.path.exists(p):
            with h5py.File(p, "r") as f:
                np.savez(os.path.join(dst_dir, os.path.splitext(name)[0] + ".npz"), **{k: np.asarray(f[k]) for k in f.keys()})


def _files_of(mode):
    return train_list if mode == 'train' else (test_list if mode == 'test' else val_list)     # pnloader.py:12-31: anything else = val


def _load(max_point, path, mode, opener, with_pid):
    datas, labels, pids = [], [], []
    for name in _files_of(mode):
        f = opener(os.path.join(path, name))
        d = np.asarray(f['data'])[:, :max_point, :]
        # channels-first float32 once, here (pnloader.py:43 does datas[i].T.astype('float32') per sample and epoch)
        datas.append(np.ascontiguousarray(np.transpose(d, (0, 2, 1)), dtype=np.float32))
        labels.append(np.asarray(f['label']).astype(np.int64))
        if with_pid:
            pids.append(np.asarray(f['pid'])[:, :max_point].astype(np.int64))
    cat = lambda xs: np.concatenate(xs, axis=0) if xs else np.zeros((0,))     # noqa: E731
    return cat(datas), cat(labels), (cat(pids) if with_pid else None)


def PNClasDataLoader(max_point=1024, batchsize=64, path='./data/', mode='train', opener=None):
    """pnloader.py:7-52.  Returns a generator function; each call = one epoch of ``(data [b,3,max_point] f32, label [b,1] i64)``."""
    datas, labels, _ = _load(max_point, path, mode, opener or default_opener, False)
    index_list = list(range(len(datas)))

    def PNClasDataGenerator():
        if mode == 'train':
            random.shuffle(index_list)                 # in place, global RNG: the reference's order for a given random.seed (pnloader.py:38-39)
        for lo in range(0, len(index_list), batchsize):
            sel = index_list[lo:lo + batchsize]
            yield datas[sel], labels[sel]

    return PNClasDataGenerator


def PNSegDataLoader(max_point=1024, batchsize=64, path='./data/', mode='train', opener=None):
    """pnloader.py:54-106.  Each call = one epoch of ``([data [b,3,max_point] f32, label [b,1] i64], target [b,max_point,1] i64)``."""
    datas, labels, pids = _load(max_point, path, mode, opener or default_opener, True)
    # np.reshape(targets[i], [max_point, -1]) (pnloader.py:95): a cloud with fewer than max_point points cannot be reshaped there either
    if len(pids) and pids.shape[1] != max_point:
        raise ValueError("cannot reshape array of size %d into shape (%d, newaxis)" % (pids.shape[1], max_point))
    targets = pids.reshape(len(pids), max_point, -1) if len(pids) else pids
    index_list = list(range(len(datas)))

    def PNSegDataGenerator():
        if mode == 'train':
            random.shuffle(index_list)
        for lo in range(0, len(index_list), batchsize):
            sel = index_list[lo:lo + batchsize]
            yield [datas[sel], labels[sel]], targets[sel]

    return PNSegDataGenerator


def kd_split_dims(points, depth):
    """tools/build_KDTree.py:6-53 (get_split_dims, build_ClasKDTree) for one cloud: points [n, 3] -> (split vectors, leaf order).

    A balanced scipy cKDTree with one point per leaf is walked depth-first, lesser child first, down to ``depth`` levels below the root.  A
    missing child stands in for by its parent (a leaf above the last level is followed as if it were its own children).  Every node above
    the last level appends its split dim TWICE to its level's vector -- where it has none (a leaf, -1) the split dim of the node it was
    reached from, or 0 if that has none either.  At the last level a node contributes one point index (drawn with np.random.choice, the
    source's call, where a leaf holds several identical points).  Returns the vectors ordered deepest level first -- lengths 2^depth,
    2^(depth-1), ... 2, int64, the order the source's dict of lists ends up in and KDNet consumes -- and the [2^depth] point indices in leaf
    order (the source's tree[-1], its level-0 point order)."""
    from scipy.spatial import cKDTree
    root = cKDTree(points, leafsize=1, balanced_tree=True).tree
    dims = [[] for _ in range(depth)]
    order = []

    def walk(node, level, parent):
        if node is None:
            node = parent
        if level >= depth:
            idx = node.indices
            if len(idx) > 1:
                idx = idx[np.random.choice(range(len(idx)), 1)]
            order.append(int(idx[0]))
            return
        walk(node.lesser, level + 1, node)
        walk(node.greater, level + 1, node)
        d = node.split_dim
        if d == -1:
            d = parent.split_dim if parent.split_dim > -1 else 0
        dims[level] += [d, d]

    walk(root, 0, None)
    return [np.asarray(v, dtype=np.int64) for v in reversed(dims)], np.asarray(order, dtype=np.int64)


def KDClasDataLoader(max_point=1024, batchsize=64, path='./data/', mode='train', opener=None):
    """kdloader.py:8-58.  The kd-tree of every cloud of the split is built once, at load time (tools/build_KDTree.py: kd_split_dims above); the
    points are stored in the tree's leaf order.  Each call of the returned function = one epoch of
    ``([points [b, 3, n] f32, split dims [b, 2n - 2] int32], label [b, 1] i64)`` with n = 2^levels, levels = log2(max_point) as the source
    takes it: a cloud's ten (for 1024 points) split vectors packed in the order KDNet consumes them, lengths n, n/2, ... 2
    (kdnet.pack_split_dims takes the batch as it comes).  The reference yields one cloud per step whatever ``batchsize`` says (kdloader.py:
    52-56); ``batchsize=1`` reproduces it, a larger one stacks that many clouds.  scipy is imported on first use."""
    levels = int((np.log(max_point) / np.log(2)).astype(int))                                      # kdloader.py:10
    opener = opener or default_opener
    points, splits, labels = [], [], []
    for name in _files_of(mode):
        f = opener(os.path.join(path, name))
        data = np.asarray(f['data'])[:, :max_point, :]
        for cloud in data:
            dims, order = kd_split_dims(cloud, levels)                                             # kdloader.py:37-41
            splits.append(np.concatenate(dims).astype(np.int32))
            points.append(np.ascontiguousarray(cloud[order].T, dtype=np.float32))                  # tree[-1].transpose(0, 2, 1), :41, :54
        labels.append(np.asarray(f['label']).astype(np.int64).reshape(len(data), -1))
    n = 1 << levels
    points = np.stack(points) if points else np.zeros((0, 3, n), np.float32)
    splits = np.stack(splits) if splits else np.zeros((0, 2 * n - 2), np.int32)
    labels = np.concatenate(labels, axis=0) if labels else np.zeros((0, 1), np.int64)
    index_list = list(range(len(points)))

    def KDClasDataGenerator():
        if mode == 'train':
            random.shuffle(index_list)                                                             # kdloader.py:49-50
        for lo in range(0, len(index_list), batchsize):
            sel = index_list[lo:lo + batchsize]
            yield [points[sel], splits[sel]], labels[sel]

    return KDClasDataGenerator


def KDSegDataLoader(max_point=1024, batchsize=64, path='./data/', mode='train', opener=None):
    """kdloader.py:60-111.  As KDClasDataLoader, with the per-point part labels (the files' ``pid``) permuted by the tree's leaf order along with
    the points (tools/build_KDTree.py:55-61).  Each call of the returned function = one epoch of
    ``([points [b, 3, n] f32, split dims [b, 2n - 2] int32], label [b, n, 1] i64)``; models.KDUNet reads the first five levels of the split
    dims.  The reference yields one cloud per step whatever ``batchsize`` says (kdloader.py:105-109); ``batchsize=1`` reproduces it."""
    levels = int((np.log(max_point) / np.log(2)).astype(int))                                      # kdloader.py:61
    opener = opener or default_opener
    n = 1 << levels
    points, splits, labels = [], [], []
    for name in _files_of(mode):
        f = opener(os.path.join(path, name))
        data = np.asarray(f['data'])[:, :max_point, :]
        pid = np.asarray(f['pid'])[:, :max_point]
        for cloud, lab in zip(data, pid):
            dims, order = kd_split_dims(cloud, levels)                                             # kdloader.py:89-91
            splits.append(np.concatenate(dims).astype(np.int32))
            points.append(np.ascontiguousarray(cloud[order].T, dtype=np.float32))                  # point_tree[-1].transpose(0, 2, 1), :92
            labels.append(lab[order].astype(np.int64).reshape(n, 1))                               # label_tree[-1].transpose(1, 0), :93, :106
    points = np.stack(points) if points else np.zeros((0, 3, n), np.float32)
    splits = np.stack(splits) if splits else np.zeros((0, 2 * n - 2), np.int32)
    labels = np.stack(labels) if labels else np.zeros((0, n, 1), np.int64)
    index_list = list(range(len(points)))

    def KDSegDataGenerator():
        if mode == 'train':
            random.shuffle(index_list)                                                             # kdloader.py:103-104
        for lo in range(0, len(index_list), batchsize):
            sel = index_list[lo:lo + batchsize]
            yield [points[sel], splits[sel]], labels[sel]

    return KDSegDataGenerator


# PAPC/datasets/tools/build_VoxData.py:4-39: the ten ModelNet categories of the voxel lists
category = {'bathtub': 0, 'bed': 1, 'chair': 2, 'door': 3, 'dresser': 4, 'airplane': 5, 'piano': 6, 'sofa': 7, 'person': 8, 'cup': 9}
categoryList = ['bathtub', 'bed', 'chair', 'door', 'dresser', 'airplane', 'piano', 'sofa', 'person', 'cup']


def VoxDataLoader(max_point=1024, batchsize=64, path='./data/', mode='train'):
    """voxloader.py:5-41.  ``path``/train.txt (``mode == 'train'``) or ``path``/test.txt lists one ``<grid .npy> <category>`` per line
    (build_VoxData.py:64-78); every grid is loaded at construction.  A grid path is opened as written -- the source's lists are relative to the
    working directory -- or, where that does not exist, relative to ``path``.  Each call of the returned function = one epoch of
    ``(grids [b, 1, 32, 32, 32] f32, label [b, 1] i64)``; train mode shuffles the order in place with the global ``random`` module
    (voxloader.py:25-26); the last batch may be short (:38-39).  ``max_point`` is unused, as in the source.  voxnet.occupancy_grid_np builds a
    grid from a cloud (build_VoxData.py:58-60)."""
    file_path = os.path.join(path, 'train.txt' if mode == 'train' else 'test.txt')               # :6-9
    datas, labels = [], []
    with open(file_path) as f:
        for data_list in f:                                                                      # :14-17
            name = data_list.split(' ')[0]
            if not os.path.isabs(name) and not os.path.exists(name):
                name = os.path.join(path, name)
            datas.append(np.load(name))
            labels.append(category[data_list.split(' ')[1].split('\n')[0]])
    datas = np.array(datas)                                                                      # :19-20
    labels = np.array(labels)
    index_list = list(range(len(datas)))

    def VoxDataGenerator():
        if mode == 'train':
            random.shuffle(index_list)                                                           # :25-26
        for lo in range(0, len(index_list), batchsize):                                          # :29-39, a batch as one gather
            sel = index_list[lo:lo + batchsize]
            yield datas[sel].reshape(len(sel), 1, 32, 32, 32).astype('float32'), labels[sel].reshape(len(sel), 1).astype('int64')

    return VoxDataGenerator


_PN_MODELS = ('pointnet_basic', 'pointnet', 'vfe', 'pointnet2_ssg', 'pointnet2_msg')


def DataLoader(model_name, max_point, batchsize, path='./data/', mode1='clas', mode2='train', opener=None):
    """dataloader.py:5-40: the dispatcher train.py calls.  The point-set models share the PN loaders and 'voxnet' gets the voxel loader
    (dataloader.py:14-15); the KD-tree loaders (KDClasDataLoader, KDSegDataLoader) are called directly and reported here as outside the
    point-set loaders."""
    if mode1 == 'clas':
        if model_name in _PN_MODELS:
            return PNClasDataLoader(max_point, batchsize, path, mode2, opener)
        if model_name == 'voxnet':
            return VoxDataLoader(max_point, batchsize, path, mode2)
        if model_name == 'kdnet':
            raise SystemExit('Error: the %s loader is outside this library (point-set models only)' % model_name)
        raise SystemExit('Error: model is incorrect')
    elif mode1 == 'seg':
        if model_name in _PN_MODELS:
            return PNSegDataLoader(max_point, batchsize, path, mode2, opener)
        if model_name == 'kdunet':
            raise SystemExit('Error: the kdunet loader is outside this library (point-set models only)')
        raise SystemExit('Error: model is incorrect')
    elif mode1 == 'detect':
        raise SystemExit('Error: Sorry, do not have detect model')
    else:
        raise SystemExit('Error: mode should be "clas", "detect" or "seg"')


def device_batches(generator, device, fps_seed=None):
    """Wrap one epoch of a PN loader for the GPU step: yields torch tensors on ``device`` -- ``(x [b,3,N] f32, y [b] i64)`` or
    ``(x, cls [b] i64, target [b,N] i64)`` -- copied through pinned host memory on the current stream.  ``fps_seed`` (optional): also yield the
    explicit FPS start indices this library takes where the reference draws them with paddle.randint (pointnet2_basic_layers.py:76), from a
    numpy generator seeded per epoch: ``(..., (s1 [b], s2 [b]))`` for the two sampling levels of the PointNet++ models."""
    import torch
    rng = np.random.default_rng(fps_seed) if fps_seed is not None else None

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if torch.device(device).type == "cuda":
            t = t.pin_memory().to(device, non_blocking=True)
        return t

    for batch in generator():
        if isinstance(batch[0], list):
            (x, cls), tgt = batch
            out = (up(x), up(cls.reshape(-1)), up(tgt.reshape(tgt.shape[0], -1)))
        else:
            x, y = batch
            out = (up(x), up(y.reshape(-1)))
        if rng is not None:
            b, n = x.shape[0], x.shape[2]
            out = out + ((up(rng.integers(0, n, size=b).astype(np.int64)), up(rng.integers(0, 512, size=b).astype(np.int64))),)
        yield out
