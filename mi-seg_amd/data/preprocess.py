"""The cached, deterministic head of the reference's transform chain on the device (data/multi_modal.py:37-49, what its CacheDataset
caches): LoadImaged + EnsureChannelFirstd + Orientationd (data/nifti.py, host) -> Spacingd (image trilinear, label nearest) ->
ScaleIntensityd -> SpatialPadd.  MONAI's own resampling grid and rounding rules are not restated (parity unpinned):
the output size is round(size * pixdim_in / pixdim_out) per axis with voxel centres aligned."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from ..hip import lib as L
from ..hip import ops
from .augment import ResidentVolume
from .decathlon import modality_id
from .nifti import ras_orientation, read_nifti, reorient_to_ras


def resample(vol, out_size, mode="trilinear"):
    """vol [C, D, H, W] on the device -> [C, *out_size]; mode 'trilinear' (fp32) | 'nearest' (any 1 / 4 / 8-byte dtype)"""
    if vol.dim() != 4 or not vol.is_cuda:
        raise ValueError("resample: device tensor [C, D, H, W] expected")
    vol = vol.contiguous()
    if mode == "trilinear":
        vol = vol.float()
    elif mode != "nearest":
        raise ValueError(f"resample: mode '{mode}'")
    out = torch.empty((vol.shape[0],) + tuple(int(s) for s in out_size), dtype=vol.dtype, device=vol.device)
    p = L.Resample3d(C.sizeof(L.Resample3d), vol.data_ptr(), out.data_ptr(), vol.shape[0], vol.shape[1], vol.shape[2], vol.shape[3], out.shape[1],
                     out.shape[2], out.shape[3], 0 if mode == "trilinear" else 1, vol.element_size())
    ops._call("miseg_resample3d", p)
    return out


def spacing(vol, pixdim_in, pixdim_out, mode):
    size = [max(1, int(round(s * pi / po))) for s, pi, po in zip(vol.shape[1:], pixdim_in, pixdim_out)]
    return resample(vol, size, mode)


def scale_intensity(img):
    """ScaleIntensityd defaults: (x - min) / (max - min) -> [0, 1] (a constant image maps to 0)"""
    lo, hi = img.amin(), img.amax()
    return (img - lo) / (hi - lo).clamp_min(1e-30)


def spatial_pad(vol, roi, value=0):
    """SpatialPadd(method="symmetric"): pad each axis up to the roi, half before / half after"""
    pads = []
    for s, r in zip(reversed(vol.shape[1:]), reversed(roi)):
        t = max(r - s, 0)
        pads += [t // 2, t - t // 2]
    return torch.nn.functional.pad(vol, pads, value=value) if any(pads) else vol


def load_resident_volume(item, pixdim=(1.0, 1.0, 1.0), roi=(96, 96, 96), device="cuda"):
    """one data-list item ({'image', 'label', 'modality'}: data/decathlon.py) -> data/augment.py::ResidentVolume, ready for the GPU
    augmenter / the sliding-window inferer"""
    img, aff = read_nifti(item["image"])
    lab, laff = read_nifti(item["label"])
    img, aff = reorient_to_ras(img, aff)
    lab, _ = reorient_to_ras(lab, laff)
    vox = np.sqrt((aff[:3, :3] ** 2).sum(0))
    image = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32))[None].to(device)
    label = torch.from_numpy(np.ascontiguousarray(lab).astype(np.int64))[None].to(device)
    image = spatial_pad(scale_intensity(spacing(image, vox, pixdim, "trilinear")), roi)
    label = spatial_pad(spacing(label, vox, pixdim, "nearest"), roi)
    return ResidentVolume(image, label[0], modality=modality_id(item.get("modality", 0)))


def nearest_index(n_in, n_out):
    """source index of each of the n_out voxels that miseg_resample3d mode 1 (nearest) reads from n_in, restated in numpy:
    floor(fma(dst + 0.5, in / out, -0.5) + 0.5) in fp32 - the kernel's multiply-add is contracted - clamped to [0, n_in).  The product and the
    difference are exact in fp64 for sides below 2^16, so one rounding to fp32 is the fused operation's."""
    a = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
    t = (a.astype(np.float64) * np.float64(np.float32(n_in) / np.float32(n_out)) - 0.5).astype(np.float32)
    return np.clip(np.floor(t + np.float32(0.5)), 0, n_in - 1).astype(np.int64)


@dataclass
class PredictionGeometry:
    """how one image's file grid maps onto the padded, resampled RAS grid the network sees (load_image_for_prediction): RAS axis k is file axis
    order[k] (reversed when flips[k]) of ras_shape[k] voxels, resampled to resampled_shape[k], then padded by pad_before[k] / pad_after[k]"""
    file_shape: tuple
    affine: np.ndarray
    order: list
    flips: list
    ras_shape: tuple
    resampled_shape: tuple
    pad_before: tuple
    pad_after: tuple

    @property
    def padded_shape(self):
        return tuple(m + b + a for m, b, a in zip(self.resampled_shape, self.pad_before, self.pad_after))

    def index_tables(self, device=None):
        """(tables, axes): for each file axis a = X, Y, Z the padded-grid index (int32, one per file voxel along a) of the logits axis axes[a]
        = the RAS axis that file axis became.  The inverse of the pad is an offset, the inverse of the spacing is the nearest rule from the
        resampled size back to the RAS size, the inverse of the orientation a flip.  With a device, the nearest rule runs as
        miseg_resample3d over an int32 arange (the kernel's own rounding); without, as nearest_index."""
        tables, axes = [None] * 3, [None] * 3
        for k, a in enumerate(self.order):
            m, n = self.resampled_shape[k], self.ras_shape[k]
            if device is not None and torch.device(device).type == "cuda":
                src = torch.arange(m, dtype=torch.int32, device=device).view(1, m, 1, 1)
                t = resample(src, (n, 1, 1), "nearest").view(n)
                t = (t.flip(0) if self.flips[k] else t) + self.pad_before[k]
            else:
                t = nearest_index(m, n)
                t = torch.from_numpy(np.ascontiguousarray(t[::-1] if self.flips[k] else t) + self.pad_before[k])
            tables[a], axes[a] = t.to(torch.int32), k
        return tables, axes

    def lerp_tables(self, mode="trilinear"):
        """(tables, axes) for hip/ops.py::soft_export: for each file axis a = X, Y, Z the triple (lo, hi, t) - the two padded-grid taps
        (int32) along the logits axis axes[a] and the fp32 weight of the hi tap, one per file voxel along a.  Built in numpy fp32 on the host.
        "trilinear": the centre-aligned rule of miseg_resample3d from the RAS size n back to the resampled size m, rounded step by step:
        f = clip((r + 0.5) * (m / n) - 0.5, 0, m - 1) with r the RAS index of the file voxel (n - 1 - i under a flip), lo = floor(f),
        hi = min(lo + 1, m - 1), t = f - lo; m == n gives lo = r and t = 0 exactly.  "nearest": lo = hi = the table of index_tables()
        (nearest_index) and t = 0, with which soft_export is the nearest gather."""
        if mode not in ("trilinear", "nearest"):
            raise ValueError(f"lerp_tables: mode {mode!r} is not one of ('trilinear', 'nearest')")
        tables, axes = [None] * 3, [None] * 3
        for k, a in enumerate(self.order):
            m, n = self.resampled_shape[k], self.ras_shape[k]
            i = np.arange(n, dtype=np.int64)
            r = n - 1 - i if self.flips[k] else i
            if mode == "nearest":
                lo = hi = nearest_index(m, n)[r]
                t = np.zeros(n, dtype=np.float32)
            else:
                scale = np.float32(m) / np.float32(n)
                f = (r.astype(np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
                f = np.clip(f, np.float32(0), np.float32(m - 1))
                lo = np.floor(f).astype(np.int64)
                hi = np.minimum(lo + 1, m - 1)
                t = f - lo.astype(np.float32)
            off = self.pad_before[k]
            tables[a] = (torch.from_numpy((lo + off).astype(np.int32)), torch.from_numpy((hi + off).astype(np.int32)),
                         torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)))
            axes[a] = k
        return tables, axes


def load_image_for_prediction(path, pixdim=(1.0, 1.0, 1.0), roi=(96, 96, 96), device="cuda"):
    """the reference's prediction transforms (predict_whs.py:46-63: Orientationd RAS, Spacingd bilinear, ScaleIntensityd, SpatialPadd) on one
    image, with the steps of load_resident_volume -> (image [1, 1, D, H, W] on the device, PredictionGeometry for the way back)"""
    img, aff = read_nifti(path)
    while img.ndim > 3 and img.shape[-1] == 1:
        img = img[..., 0]
    if img.ndim != 3:
        raise ValueError(f"{path}: a 3-D image expected, got shape {img.shape}")
    order, flips = ras_orientation(aff)
    ras, ras_aff = reorient_to_ras(img, aff)
    vox = np.sqrt((ras_aff[:3, :3] ** 2).sum(0))
    image = torch.from_numpy(np.ascontiguousarray(ras, dtype=np.float32))[None].to(device)
    image = scale_intensity(spacing(image, vox, pixdim, "trilinear"))
    resampled = tuple(int(s) for s in image.shape[1:])
    image = spatial_pad(image, roi)
    before = tuple(max(r - s, 0) // 2 for s, r in zip(resampled, roi))
    after = tuple(max(r - s, 0) - b for s, r, b in zip(resampled, roi, before))
    geom = PredictionGeometry(tuple(int(s) for s in img.shape), np.asarray(aff, dtype=np.float64), list(order), list(flips), tuple(int(s) for s in ras.shape),
                              resampled, before, after)
    return image[None], geom
