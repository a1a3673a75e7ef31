"""Keep-largest-connected-component post-processing: MONAI 1.1.0 transforms/post/array.py::KeepLargestConnectedComponent and
transforms/utils.py::get_largest_connected_component_mask restated (parity unpinned: neither MONAI nor skimage is a dependency; DESIGN.md
section 7.7 writes the rules down).  On a HIP device the class map goes through csrc/components.hip (hip/ops.py::keep_largest_component);
CPU tensors take keep_largest_numpy below, the restatement the device tests compare against.

The rules: `applied` classes are filtered, every other value is left alone and connects nothing.  independent: per applied class c the
components of {cls == c}; joint: the components of {cls in applied}, adjacent applied voxels of different classes connected.  The largest
component stays (among equals the one holding the smallest linear voxel index), every other voxel of the group becomes 0.  connectivity
1 / 2 / 3 (None = 3): 6 / 18 / 26 neighbours, never across the end of a row, slice or sample.

Fill-holes (MONAI 1.1.0 transforms/post/array.py::FillHoles and transforms/utils.py::fill_holes restated): FillHoles,
fill_holes_numpy and, on a HIP device, hip/ops.py::fill_holes.  The applied labels (never 0) are taken in ascending order, each on the map as
the previous one left it; for label L the voxels that are not L are connected through the chosen neighbourhood, a component that holds a voxel
on a face of the volume is open, and every voxel of every other component becomes L."""
import numpy as np
import torch

MAX_CLASSES = 64


def _ndimage():
    try:
        from scipy import ndimage
        return ndimage
    except ImportError:
        return None


def check_connectivity(connectivity):
    c = 3 if connectivity is None else int(connectivity)
    if c not in (1, 2, 3):
        raise ValueError(f"connectivity {connectivity!r}: 1, 2, 3 or None (= 3)")
    return c


def applied_mask(applied_labels, num_classes):
    """the 64-bit set of filtered classes: every class but 0 by default"""
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"num_classes {num_classes} (1..{MAX_CLASSES})")
    if applied_labels is None:
        return ((1 << num_classes) - 1) & ~1
    if isinstance(applied_labels, (int, np.integer)):
        applied_labels = [applied_labels]
    mask = 0
    for c in applied_labels:
        if int(c) != c or not 0 <= int(c) < num_classes:
            raise ValueError(f"applied label {c!r} is not a class of [0, {num_classes})")
        mask |= 1 << int(c)
    return mask


def _offsets(connectivity):
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < (a != 0) + (b != 0) + (c != 0) <= connectivity]


def label_components_numpy(mask, connectivity):
    """exact labelling without scipy: every voxel of the bool volume `mask` gets the smallest linear index of its component (mask.size
    outside the mask).  Min-index propagation over the shifted neighbours, with pointer jumping (a label is the index of a voxel of the same
    component, so that voxel's label is one too), until nothing changes."""
    n = mask.size
    lab = np.where(mask, np.arange(n, dtype=np.int64).reshape(mask.shape), n)
    flat, m = lab.reshape(-1), mask.reshape(-1)
    pairs = []
    for off in _offsets(connectivity):
        dst = tuple(slice(max(o, 0), s + min(o, 0)) for o, s in zip(off, mask.shape))
        src = tuple(slice(max(-o, 0), s + min(-o, 0)) for o, s in zip(off, mask.shape))
        if all(s.stop > s.start for s in dst):
            pairs.append((dst, src))
    while True:
        before = lab.copy()
        for dst, src in pairs:
            lab[dst] = np.where(mask[dst], np.minimum(lab[dst], lab[src]), n)
        for _ in range(4):
            flat[m] = flat[flat[m]]
        if np.array_equal(before, lab):
            return lab


def _components(mask, connectivity, nd):
    """(labels of the masked voxels in raster order, their linear indices): any numbering"""
    idx = np.flatnonzero(mask)
    if nd is not None:
        lab, _ = nd.label(mask, nd.generate_binary_structure(mask.ndim, connectivity))
    else:
        lab = label_components_numpy(mask, connectivity)
    return lab.reshape(-1)[idx], idx


def _largest(mask, connectivity, nd):
    """bool volume of the largest component of `mask` (ties: the smallest first linear index) and the first indices of all components"""
    labels, idx = _components(mask, connectivity, nd)
    ids, first, counts = np.unique(labels, return_index=True, return_counts=True)      # idx ascends: the first occurrence is the smallest index
    win = ids[np.lexsort((idx[first], -counts))[0]]
    keep = np.zeros(mask.shape, dtype=bool)
    keep.reshape(-1)[idx[labels == win]] = True
    return keep, idx[first]


def get_largest_connected_component_mask(img, connectivity=None, num_components=1, use_scipy=True):
    """bool array of img's shape (up to 3 spatial dims): the largest connected component of img != 0 (empty if img has none)"""
    if num_components != 1:
        raise NotImplementedError(f"num_components = {num_components}: only the largest component (1) is implemented")
    conn = check_connectivity(connectivity)
    tensor = isinstance(img, torch.Tensor)
    arr = img.detach().cpu().numpy() if tensor else np.asarray(img)
    mask = arr.astype(bool)
    if mask.ndim > 3:
        raise ValueError(f"get_largest_connected_component_mask: {mask.ndim} spatial dimensions (at most 3)")
    vol = mask.reshape((1,) * (3 - mask.ndim) + mask.shape)
    # leading axes of size 1 have no neighbours: a connectivity above the image's own dimension count acts as that count, as in skimage
    keep = _largest(vol, conn, _ndimage() if use_scipy else None)[0] if vol.any() else np.zeros_like(vol)
    keep = keep.reshape(mask.shape)
    return torch.from_numpy(keep).to(img.device) if tensor else keep


def keep_largest_numpy(cls, num_classes, applied_labels=None, independent=True, connectivity=None, use_scipy=True, return_stats=False):
    """the device op's restatement on an integer class map [B, D, H, W] (or [D, H, W]): a copy with the dropped voxels at 0.  Values outside
    [0, num_classes) are left alone.  use_scipy=False takes the numpy labelling even where scipy imports.  return_stats: also int64 [B, C, 3]
    = voxels of class c before, kept, and components whose first voxel has class c (applied classes only)."""
    conn = check_connectivity(connectivity)
    applied = applied_mask(applied_labels, num_classes)
    nd = _ndimage() if use_scipy else None
    cls = np.asarray(cls)
    single = cls.ndim == 3
    vols = cls[None] if single else cls
    if vols.ndim != 4:
        raise ValueError(f"keep_largest_numpy: class map of shape {cls.shape} ([B,] D, H, W)")
    out = vols.copy()
    stats = np.zeros((vols.shape[0], num_classes, 3), dtype=np.int64)
    classes = [c for c in range(num_classes) if (applied >> c) & 1]
    for b, vol in enumerate(vols):
        groups = [vol == c for c in classes] if independent else [np.isin(vol, classes)] if classes else []
        dropped = np.zeros(vol.shape, dtype=bool)
        for mask in groups:
            if not mask.any():
                continue
            keep, first = _largest(mask, conn, nd)
            dropped |= mask & ~keep
            stats[b, :, 2] += np.bincount(vol.reshape(-1)[first], minlength=num_classes)[:num_classes]
        out[b][dropped] = 0
        for c in range(num_classes):
            stats[b, c, 0] = np.count_nonzero(vol == c)
            stats[b, c, 1] = np.count_nonzero((vol == c) & ~dropped)
    out = out[0] if single else out
    return (out, stats[0] if single else stats) if return_stats else out


def fill_labels(applied_labels, num_classes):
    """the ascending list of filled labels: every class but 0 by default; 0, the background, is discarded"""
    applied = applied_mask(applied_labels, num_classes) & ~1
    return [c for c in range(1, num_classes) if (applied >> c) & 1]


def _enclosed(passable, connectivity, nd):
    """bool volume of the passable voxels in components that touch no face of the 3-d volume `passable`"""
    if nd is not None:          # MONAI's recipe, literally: grow an empty seed from the border through the mask until nothing changes
        tmp = np.zeros(passable.shape, dtype=bool)
        nd.binary_dilation(tmp, structure=nd.generate_binary_structure(3, connectivity), iterations=-1, mask=passable, origin=0, border_value=1,
                           output=tmp)
        return passable & ~tmp
    lab = label_components_numpy(passable, connectivity)
    face = np.zeros(passable.shape, dtype=bool)
    for ax in range(3):
        sl = [slice(None)] * 3
        for end in (0, -1):
            sl[ax] = end
            face[tuple(sl)] = True
    open_roots = np.unique(lab[face & passable])
    return passable & ~np.isin(lab, open_roots)


def fill_holes_numpy(cls, num_classes, applied_labels=None, connectivity=None, use_scipy=True, return_stats=False):
    """the device op's restatement on an integer class map [B, D, H, W] (or [D, H, W]): a copy with the holes of every applied label filled.
    A value outside [0, num_classes) is passable like any other and is overwritten inside a hole.  use_scipy=False takes the numpy labelling
    plus a face flag even where scipy imports.  return_stats: also int64 [B, C] = voxels whose value the pass of label c changed to c."""
    conn = check_connectivity(connectivity)
    labels = fill_labels(applied_labels, num_classes)
    nd = _ndimage() if use_scipy else None
    cls = np.asarray(cls)
    single = cls.ndim == 3
    vols = cls[None] if single else cls
    if vols.ndim != 4:
        raise ValueError(f"fill_holes_numpy: class map of shape {cls.shape} ([B,] D, H, W)")
    out = vols.copy()
    stats = np.zeros((vols.shape[0], num_classes), dtype=np.int64)
    for b in range(out.shape[0]):
        vol = out[b]
        for c in labels:
            passable = vol != c
            if passable.all() or min(vol.shape) == 1:      # an absent label has no holes; with a side of 1 every voxel lies on a face
                continue
            hole = _enclosed(passable, conn, nd)
            stats[b, c] = np.count_nonzero(hole)
            vol[hole] = c
    out = out[0] if single else out
    return (out, stats[0] if single else stats) if return_stats else out


def _class_volume(img):
    """one-channel sample [1, *spatial] -> (int32 [1, D, H, W] with -1 wherever the value is non-integral: no class / label; the spatial shape)"""
    cls = img.reshape((1,) * (5 - img.dim()) + img.shape[1:])      # leading spatial axes of size 1 are added
    whole = cls.to(torch.int32)
    return torch.where(whole.to(cls.dtype) == cls, whole, torch.full_like(whole, -1)).contiguous(), img.shape[1:]


def _applied_channels(img, applied_labels):
    """index tensor of the applied channels of a one-hot sample [C, *spatial] (default: all but channel 0), validated; None if there are none"""
    applied = tuple(range(1, img.shape[0])) if applied_labels is None else applied_labels
    if any(not 0 <= c < img.shape[0] for c in applied):
        raise ValueError(f"applied labels {applied} for {img.shape[0]} channels")
    return torch.as_tensor(applied, device=img.device) if applied else None


def _binary_batch(op, maps, connectivity):
    """bool [N, *spatial] through the device op `op` as N samples of two classes (leading spatial axes of size 1 added) -> its result in maps' shape"""
    vol = maps.reshape(maps.shape[:1] + (1,) * (4 - maps.dim()) + maps.shape[1:]).to(torch.uint8).contiguous()
    return op(pred=vol, num_classes=2, applied_labels=(1,), connectivity=connectivity).reshape(maps.shape)


class FillHoles:
    """monai.transforms.FillHoles on one channel-first sample [C, *spatial] (up to 3 spatial dims; leading spatial axes of size 1 are added, so a
    sample of fewer dims has a side of 1 and is returned as it is).  One channel: a class map of the labels 1..63 (applied_labels default: all of
    them); values of 64 and above and non-integral values are passable like any other voxel, are overwritten inside a hole, and are no labels
    themselves.  Several channels: one-hot - every applied channel (default: all but channel 0) is a binary map of its own (non-zero = the
    label), sent through as an extra batch entry with two classes; as in MONAI the channel comes back as 0 / 1.  Device tensors go through the
    fill-holes kernels, CPU tensors through fill_holes_numpy."""

    def __init__(self, applied_labels=None, connectivity=None):
        if isinstance(applied_labels, (int, np.integer)):
            applied_labels = [applied_labels]
        self.applied_labels = None if applied_labels is None else tuple(sorted({int(c) for c in applied_labels} - {0}))
        self.connectivity = connectivity
        check_connectivity(connectivity)

    def class_map(self, logits=None, pred=None, num_classes=None, out_dtype=torch.int32, stats=False):
        """the filter on a batch: fp32 logits [B, C, D, H, W] (first-maximum argmax) or an integer class map [B, D, H, W] -> [B, D, H, W]"""
        from ..hip import ops
        return ops.fill_holes(logits=logits, pred=pred, num_classes=num_classes, applied_labels=self.applied_labels, connectivity=self.connectivity,
                              out_dtype=out_dtype, stats=stats)

    def __call__(self, img):
        from ..hip import ops
        if not isinstance(img, torch.Tensor):
            img = torch.as_tensor(img)
        if img.dim() < 2 or img.dim() > 4:
            raise ValueError(f"FillHoles: a channel-first sample [C, *spatial] with 1..3 spatial dims, got {tuple(img.shape)}")
        out = img.clone()
        if img.shape[0] == 1:
            whole, sp = _class_volume(img)
            res = self.class_map(pred=whole, num_classes=MAX_CLASSES)
            changed = (res != whole).reshape(sp)
            out[0][changed] = res.reshape(sp)[changed].to(img.dtype)
            return out
        idx = _applied_channels(img, self.applied_labels)
        if idx is None:
            return out
        out[idx] = _binary_batch(ops.fill_holes, img[idx] != 0, self.connectivity).to(img.dtype)
        return out


class KeepLargestConnectedComponent:
    """monai.transforms.KeepLargestConnectedComponent on one channel-first sample [C, *spatial] (up to 3 spatial dims).  One channel: a class
    map (applied_labels default: every value of 1..63; values of 64 and above are left alone).  is_onehot, or more than one channel: every applied
    channel (default: all but channel 0) is a binary map of its own - independent: each keeps its largest component; joint: the largest component
    of their union stays in every applied channel.  Device tensors go through the keep-largest kernels (a one-hot sample as extra batch entries
    with two classes), CPU tensors through keep_largest_numpy."""

    def __init__(self, applied_labels=None, is_onehot=None, independent=True, connectivity=None, num_components=1):
        if num_components != 1:
            raise NotImplementedError(f"num_components = {num_components}: only the largest component (1) is implemented")
        if isinstance(applied_labels, (int, np.integer)):
            applied_labels = [applied_labels]
        self.applied_labels = None if applied_labels is None else tuple(int(c) for c in applied_labels)
        self.is_onehot, self.independent, self.connectivity, self.num_components = is_onehot, bool(independent), connectivity, 1
        check_connectivity(connectivity)

    def class_map(self, logits=None, pred=None, num_classes=None, out_dtype=torch.int32, stats=False):
        """the filter on a batch: fp32 logits [B, C, D, H, W] (first-maximum argmax) or an integer class map [B, D, H, W] -> [B, D, H, W]"""
        from ..hip import ops
        return ops.keep_largest_component(logits=logits, pred=pred, num_classes=num_classes, applied_labels=self.applied_labels,
                                          independent=self.independent, connectivity=self.connectivity, out_dtype=out_dtype, stats=stats)

    def __call__(self, img):
        if not isinstance(img, torch.Tensor):
            img = torch.as_tensor(img)
        if img.dim() < 2 or img.dim() > 4:
            raise ValueError(f"KeepLargestConnectedComponent: a channel-first sample [C, *spatial] with 1..3 spatial dims, got {tuple(img.shape)}")
        is_onehot = img.shape[0] > 1 if self.is_onehot is None else bool(self.is_onehot)
        out = img.clone()
        if not is_onehot:
            if img.shape[0] != 1:
                raise ValueError(f"KeepLargestConnectedComponent: a class map has one channel, got {img.shape[0]}")
            whole, sp = _class_volume(img)
            res = self.class_map(pred=whole, num_classes=MAX_CLASSES)
            out[0][((res == 0) & (whole > 0)).reshape(sp)] = 0
            return out
        idx = _applied_channels(img, self.applied_labels)
        if idx is None:
            return out
        from ..hip import ops
        fg = img[idx] > 0
        maps = fg if self.independent else (img[idx] == 1).any(0, keepdim=True)      # each channel's own map, or the union of them
        drop = maps & (_binary_batch(ops.keep_largest_component, maps, self.connectivity) == 0)
        out[idx] = torch.where(drop.expand_as(fg), torch.zeros_like(img[idx]), img[idx])
        return out
