"""The table of README.md ("Giving the texture a prior"): what the pixel terms leave undetermined in the texture, on the CPU oracle.
The 128 x 128 scene (the 1k mesh, a 256 x 256 x 1 texture), cameras 0 and 4, two frames at the ground truth, float32 oracle operators.

  1. The share of the chart's texels (the texels the render can read: the UV triangles rasterised at the texture's resolution, grown
     by one texel) whose pixel-term gradient is EXACTLY 0 from a random texture -- no covered pixel of any image taps them --, and the
     same when a disc in the middle of every image is masked out.
  2. The locally normalised loss (tests/norm_ref.py, sigma 4, kernel 15, eps 2) and the plain pixel loss when the texture is replaced by
     1.25 t + 0.05, against the anchor term of the Texture prior rule for that change, per unit weight.

    python scripts/tex_prior_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS, N_FRAMES, DISC = (0, 4), 2, 0.25       # the disc's radius as a share of the image's height


def main():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import blur_ref
    import norm_ref
    import tex_prior_ref as T
    from fpc_diffrend_amd import scene
    from oracle import fit as ofit, ops as oops
    sc = scene.make_scene(n_frames=N_FRAMES, resolution=(128, 128))
    H, W = sc.resolution
    Ht, Wt, _ = sc.texture.shape

    def state(texture):
        st = ofit.State(sc, CAMS, texture=texture, n_frames=N_FRAMES)
        with torch.no_grad():
            st.M1.copy_(torch.eye(N_FRAMES))
            st.M2.copy_(torch.tensor(sc.weights_gt[:N_FRAMES]).t())
            st.per_frame_t.copy_(torch.tensor(sc.t_gt[:N_FRAMES]))
        return st

    def render(texture):
        st = state(texture)
        pos_clip, _ = ofit.clip_positions(st, torch.arange(N_FRAMES))
        zero = torch.zeros(N_FRAMES * len(CAMS), H, W, dtype=torch.uint8)
        _, image, rast = ofit.forward_from_clip(st, pos_clip, zero)
        return st, image, rast

    # the captures: the ground truth rendered with the true texture
    _, image, rast = render(sc.texture)
    ref = torch.round(image.detach() * 255.0).clamp(0, 255).to(torch.uint8)[..., 0]
    cover = rast[..., 3] > 0
    uv, uv_idx = torch.tensor(sc.uv), torch.tensor(sc.uv_idx)
    pos = torch.stack([2 * uv[:, 0] - 1, 2 * uv[:, 1] - 1, torch.zeros(uv.shape[0]), torch.ones(uv.shape[0])], dim=1)
    chart = T.dilate3(oops.rasterize_ids(pos[None], uv_idx, (Ht, Wt))[0].numpy() > 0)
    print(f"scene: {H} x {W}, cameras {CAMS}, {N_FRAMES} frames, texture {Ht} x {Wt}; the mesh covers {float(cover.float().mean()):.1%} of the "
          f"pixels; chart: {int(chart.sum())} of {Ht * Wt} texels")

    # 1. texels without a gradient, from a random texture
    noise = np.random.default_rng(0).uniform(size=sc.texture.shape).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = torch.tensor(((yy - H / 2) ** 2 + (xx - W / 2) ** 2) <= (DISC * H) ** 2)
    for name, weight in (("no mask", torch.ones(H, W)), (f"a disc of radius {DISC:g} H masked out", (~disc).float())):
        st, img, _ = render(noise)
        loss = (weight[None, :, :, None] * (ref[..., None].float() - img * 255.0) ** 2).mean()
        loss.backward()
        dead = (st.tex.grad.abs().sum(dim=2) == 0).numpy() & chart
        print(f"chart texels whose pixel-term gradient is exactly 0, {name}: {int(dead.sum())} of {int(chart.sum())} ({dead.sum() / chart.sum():.1%})")

    # 2. what the normalised loss does not see
    g = blur_ref.taps(15, 4.0)
    t0 = torch.tensor(sc.texture)
    t1 = 1.25 * t0 + 0.05
    rows = []
    for tex in (t0, t1):
        _, img, _ = render(tex.numpy())
        colour = img.detach()
        plain = float(((ref[..., None].float() - colour * 255.0) ** 2).mean())
        norm = float(norm_ref.loss_plain(colour.double(), cover, ref, g.double(), eps=2.0))
        rows.append((plain, norm))
    anchor = float(T.tex_prior(t1, 0.0, 1.0, anchor=t0)['part'][0][1])
    print(f"texture t -> 1.25 t + 0.05: plain pixel loss {rows[0][0]:.4g} -> {rows[1][0]:.4g}; normalised loss {rows[0][1]:.4g} -> {rows[1][1]:.4g}; "
          f"anchor term per unit weight 0 -> {anchor:.4g}")


if __name__ == "__main__":
    main()
