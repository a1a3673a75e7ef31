#!/usr/bin/env python3
"""Generate tests/golden/unet_vanilla.npz by running the REFERENCE's conditional UNet (networks/nets/unet_vanilla.py) on the CPU.

Needs a checkout of the reference project (MISEG_REFERENCE points at it, as for oracle/tools/make_golden.py):

    python scripts/make_golden_unet_vanilla.py

oracle/tools/make_golden.py is loaded by path and reused as it stands: its reference / MONAI stand-in import paths, the instance-norm
gradient workaround it installs, the norm configurations, whole_net and save.  The fixture holds data only.

Cases
  cond_32    channels [8, 16, 32, 64], strides [1, 2, 2, 1], 2 residual units, instance_cond down / instance up, x (2, 1, 32^3),
             modalities [1, 0], 8 classes.  The full logits (2 MiB of fp32) would break the size limit of a committed file: the logits
             of every class at the voxels [::2, ::2, ::4] (`logits_sub`, 128 KiB) stand in for them, beside whole_net's strided samples and
             l2 norm.
  pre_s2     channels [8, 16, 32], strides [2, 2, 2], instance norms, x (1, 1, 32^3): the stride-2 pre_conv on the raw image, logits at 16^3
             (stored whole).
  published  the README's configuration (feature_size 16 64 128 256 512, strides 1 2 2 2 1, 3 residual units, 8 classes): state keys,
             shapes and parameter count only, no forward.
"""
import copy
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "tools", "make_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

from networks.nets.unet_vanilla import UNetVanilla  # noqa: E402  (reference, on the path make_golden.py set up)

OUT_CHANNELS = 8
PUBLISHED = dict(channels=[16, 64, 128, 256, 512], strides=[1, 2, 2, 2, 1], num_res_units=3)


def build(channels, strides, num_res_units, norm_down, norm_up):
    return UNetVanilla(3, 1, OUT_CHANNELS, channels=channels, strides=strides, num_res_units=num_res_units, act="prelu",
                       norm_down=copy.deepcopy(norm_down), norm_up=copy.deepcopy(norm_up), dropout=0.0, bias=True, adn_ordering="NDA")


def main():
    arrays, meta = {}, {"cases": {}}
    c = dict(channels=[8, 16, 32, 64], strides=[1, 2, 2, 1], num_res_units=2)
    m = build(**c, norm_down=MG.COND, norm_up=MG.INST)
    MG.whole_net("cond_32", m, (2, 1, 32, 32, 32), [1, 0], dict(c, norm_down="instance_cond", norm_up="instance"), False, [], arrays, meta)
    # whole_net does not hand its logits back: the subsampled ones come from a second forward of the same filled module
    import torch
    with torch.no_grad():
        y = m(MG.det_input(1234, (2, 1, 32, 32, 32)), [1, 0])
    arrays["cond_32/logits_sub"] = MG.np32(y[:, :, ::2, ::2, ::4])

    c = dict(channels=[8, 16, 32], strides=[2, 2, 2], num_res_units=2)
    m = build(**c, norm_down=MG.INST, norm_up=MG.INST)
    MG.whole_net("pre_s2", m, (1, 1, 32, 32, 32), None, dict(c, norm_down="instance", norm_up="instance"), False, [], arrays, meta)

    m = build(**PUBLISHED, norm_down=MG.COND, norm_up=MG.INST)
    sd = m.state_dict()
    meta["cases"]["published"] = dict(PUBLISHED, norm_down="instance_cond", norm_up="instance", out_channels=OUT_CHANNELS,
                                      state_keys=list(sd.keys()), state_shapes=[list(v.shape) for v in sd.values()],
                                      n_params=sum(p.numel() for p in m.parameters()), n_state=len(sd))
    print(f"    published: params {meta['cases']['published']['n_params']} state entries {len(sd)}")
    meta["unpinned"] = []
    MG.save("unet_vanilla", arrays, meta)


if __name__ == "__main__":
    main()
