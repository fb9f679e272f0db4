"""The README's landmark table: float64 on the CPU, the oracle's pixel term beside the landmark term (tests/landmark_ref.py, the statement
of DESIGN.md 3, "Landmark rule") as the head is moved off its place.

scene.make_scene(resolution=(128, 128), n_frames=1), cameras (0, 4), everything at the hidden truth; the targets are the oracle's own
render, quantised; the landmarks are fit.project_landmarks on every thirteenth vertex (40 of 514, no occlusion reasoning, confidence 1);
frame 0 is moved along per_frame_t[0, 0] by d full-size pixels (1 unit = 3.494 px, as the README's other scans have it).  Per d: the
plain pixel loss and its derivative along the axis, the landmark term at weight 1 (mean squared reprojection error in pixels^2) and its
derivative.  ONE scene and ONE axis: the reason for the design, not a promise about real takes.

    python scripts/landmark_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = 3.494
OFFSETS = (-40, -20, -8, -2, 0, 2, 8, 20, 40)
CAMS = (0, 4)


def rows():
    """One dict per offset d: 'd', 'pix' and 'pix_slope' (the pixel loss and d loss / d per_frame_t[0, 0]), 'lmk' and 'lmk_slope' (the
    landmark term at weight 1), 'live' (the landmarks that count, of 2 x 40)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import landmark_ref as LR
    from fpc_diffrend_amd import fit, scene
    from oracle import fit as ofit
    from oracle import ops as oracle_ops
    oracle_ops.build()
    sc = scene.make_scene(resolution=(128, 128), n_frames=1)
    H, W = sc.resolution
    points = [{'vertex': v} for v in range(0, sc.n_vertices, 13)]
    obs = torch.tensor(fit.project_landmarks(sc, points, CAMS)).reshape(len(CAMS), len(points), 3)
    vtx, bary, _ = LR.tables(points, sc.n_vertices, sc.pos_idx)

    def state(d):
        st = ofit.State(sc, cams=list(CAMS), dtype=torch.float64)
        with torch.no_grad():
            st.M1.copy_(torch.eye(1))
            st.M2.copy_(torch.tensor(sc.weights_gt).t())
            st.per_frame_t.copy_(torch.tensor(sc.t_gt))
            st.per_frame_q.copy_(torch.tensor(sc.q_gt))
            st.per_frame_t[0, 0] += d / PX
        return st

    def chain(st):      # (pos_clip, verts, mvp): the oracle's own matrices, recovered from its clip positions' chain
        frame_ids = torch.arange(1)
        pos_clip, verts = ofit.clip_positions(st, frame_ids)
        cs = torch.tensor(st.cams)
        rc = ofit.rigid(st.t_opt[cs], ofit.quat_to_rotmat(st.q_opt[cs]))
        rf = ofit.rigid(st.per_frame_t[frame_ids], ofit.quat_to_rotmat(st.per_frame_q[frame_ids]))
        mvp = torch.matmul(st.P[None], torch.matmul(rf[:, None], torch.matmul(rc, st.TMV)[None])).reshape(len(CAMS), 4, 4)
        return pos_clip, verts, mvp

    with torch.no_grad():
        pos_clip, _, _ = chain(state(0.0))
        _, image, _ = ofit.forward_from_clip(state(0.0), pos_clip, torch.zeros(len(CAMS), H, W, dtype=torch.uint8))
        targets = torch.round(image[..., 0] * 255.0).clamp(0, 255).to(torch.uint8)
    out = []
    for d in OFFSETS:
        st = state(float(d))
        pos_clip, verts, mvp = chain(st)
        pix, _, _ = ofit.forward_from_clip(st, pos_clip, targets)
        g_pix, = torch.autograd.grad(pix, st.per_frame_t, retain_graph=True)
        lmk = LR.landmark_plain(verts, mvp, vtx, bary, None, obs, 1.0, H, W)
        g_lmk, = torch.autograd.grad(lmk, st.per_frame_t)
        # the closed form of the statement gives the same number as the differentiable restatement
        ref = LR.landmark(verts.detach(), mvp.detach(), vtx, bary, None, obs, 1.0, H, W, grads=False)
        assert abs(float(ref['value'][0]) - float(lmk.detach())) <= 1e-9 * max(1.0, float(lmk.detach()))
        out.append(dict(d=d, pix=float(pix.detach()), pix_slope=float(g_pix[0, 0]), lmk=float(lmk.detach()), lmk_slope=float(g_lmk[0, 0]),
                        live=int(ref['live'].sum())))
    return out


def format_row(r):
    """The row of the README's table."""
    d = "0" if r['d'] == 0 else f"{r['d']:+d}".replace("-", "−")
    num = lambda v, f: format(v, f).replace("-", "−")
    return f"| {d} | {r['pix']:.3f} (g {num(r['pix_slope'], '+.3g')}) | {r['lmk']:.2f} (g {num(r['lmk_slope'], '+.1f')}) |"


if __name__ == "__main__":
    print("| d | pixel loss | landmark term, weight 1 |")
    print("|---|---|---|")
    for r in rows():
        print(format_row(r))
