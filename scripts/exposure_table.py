"""The Exposure rule on the CPU oracle -> the table of README.md: needs no GPU.  The README's exposure scene --
scene.make_scene(resolution=(128, 128), n_frames=1), cameras (0, 4), everything at the hidden truth, targets the oracle's own render
quantised, camera 0's replaced by round(0.75 x + 8) and camera 4's by round(1.25 x - 6) -- with frame 0 moved along per_frame_t[0, 0] by
d = 0, 1, 2, 4 full-size pixels (1 unit = 3.494 px) before the render the gains are fitted against.  For both methods: the recovered
a_c, b_c, rho_c and g_c, and at d = 0 the plain pixel loss before and after the captures are mapped, next to the loss with equal
exposures.  The sums are the numpy statement's (tests/exposure_ref.py), the fit is exposure.fit_gains.

    python scripts/exposure_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import exposure_ref as R
from fpc_diffrend_amd import exposure, scene
from oracle import fit as ofit
from oracle import ops as oracle_ops

PX = 3.494
CAMS = [0, 4]


def main():
    oracle_ops.build()
    sc = scene.make_scene(resolution=(128, 128), n_frames=1)

    def state(d):
        st = ofit.State(sc, cams=CAMS)
        with torch.no_grad():
            st.M1.copy_(torch.eye(1))
            st.M2.copy_(torch.tensor(sc.weights_gt).t())
            st.per_frame_t.copy_(torch.tensor(sc.t_gt))
            st.per_frame_q.copy_(torch.tensor(sc.q_gt))
            st.per_frame_t[0, 0] += d / PX
        return st

    def render(d, targets):
        with torch.no_grad():
            st = state(d)
            pos_clip, _ = ofit.clip_positions(st, torch.arange(1))
            return ofit.forward_from_clip(st, pos_clip, targets)

    _, image, _ = render(0.0, torch.zeros(2, 128, 128, dtype=torch.uint8))
    x = torch.round(image[..., 0] * 255.0)
    equal = x.clamp(0, 255).to(torch.uint8)
    gains = torch.stack([torch.round(0.75 * x[0] + 8.0), torch.round(1.25 * x[1] - 6.0)]).clamp(0, 255).to(torch.uint8)
    loss_equal = float(render(0.0, equal)[0])
    loss_before = float(render(0.0, gains)[0])
    print(f"plain pixel loss at the truth: equal exposures {loss_equal:.3f}, with the gains {loss_before:.3f}")
    print("| d (px) | method | a0, a4 | b0, b4 | rho0, rho4 | g0, g4 | g0 / g4 (truth 1.667) | loss at d = 0 after |")
    print("|---|---|---|---|---|---|---|---|")
    for d in (0, 1, 2, 4):
        _, image, rast = render(float(d), gains)
        table = R.sums(image.numpy(), rast.numpy(), gains.numpy(), lo=1, hi=254)      # one image a camera: the rows are the cameras
        for method in exposure.METHODS:
            out = exposure.fit_gains(table, method=method)
            after = ""
            if d == 0:
                mapped = torch.from_numpy(R.apply(gains.numpy().reshape(2, -1), out['lut'], [0, 1]).reshape(2, 128, 128))
                after = f"{float(render(0.0, mapped)[0]):.3f}"
            f2 = lambda v: ", ".join(f"{u:.3f}" for u in v)
            print(f"| {d} | {method} | {f2(out['a'])} | {f2(out['b'])} | {f2(out['rho'])} | {f2(out['g'])} | {out['g'][0] / out['g'][1]:.4f} | {after} |")


if __name__ == "__main__":
    main()
