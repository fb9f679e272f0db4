"""HIP-event time of fpcdr_robust_loss (the weighted robust pixel loss, csrc/robust.hip) on a batch of 18 images of 1080 x 1920 (one
channel): each kind, with and without mask and face weights, value only and with the gradient, beside fpcdr_pixel_loss on the same
tensors -- this library's in the same process, the variants taking turns, and, with --parent DIR, the one of another build of the package
(the parent commit's, exported and built under DIR) in a process of its own.  Before timing, value and gradient are held against the torch
statement of the rule (tests/robust_ref.py's loss_plain) on a crop of the batch.

Algorithmic bytes per pixel of a call with C channels: colour (4 C), the coverage record (16: the kernel uses rast.w only, the memory
moves the record's lines whole), the capture (1), the mask (1, when given), the gradient (4 C, when asked for); the face-weight table
(4 T bytes) stays in the caches.  fpcdr_pixel_loss: 8 C + 17.

--fitter: one line for a whole Fitter step at cfg3's shape (32 frames x 9 cameras of 1080 x 1920, 30 k triangles) on the robust term
(Charbonnier, c = 10, a mask) beside the fused_objective=False L2 step and the default one-pass step; with --parent DIR the
fused_objective=False step of that build too.

    python scripts/robust_time.py [--commit NAME] [--seconds S] [--parent DIR] [--fitter]
"""
import dataclasses
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (18, 1080, 1920, 1)
T_FACES = 30000
SCALE = 10.0
HBM_PEAK = 8.0e12        # bytes/s, MI355X spec


def _tensors():
    import torch
    B, H, W, C = SHAPE
    g = torch.Generator().manual_seed(0)
    colour = torch.rand(B, H, W, C, generator=g).cuda()
    rast = torch.zeros(B, H, W, 4, device='cuda')
    ids = torch.randint(1, T_FACES + 1, (B, H, W), generator=g).float()
    ids[torch.rand(B, H, W, generator=g) < 0.4] = 0.0
    rast[..., 3] = ids.cuda()
    ref = torch.randint(0, 141, (B, H, W), generator=g, dtype=torch.uint8).cuda()
    mask = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8).cuda()
    face_w = (torch.rand(T_FACES, generator=g) * 1.5).cuda()
    return colour, rast, ref, mask, face_w


def _take_turns(variants, seconds, calls=2):
    """name -> sorted per-call milliseconds: HIP events around `calls` calls of one variant, the variants taking turns."""
    import numpy as np
    import torch
    for _, _, fn in variants:                  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    turns = {name: [] for name, _, _ in variants}
    t0 = time.perf_counter()
    while min(sum(v) for v in turns.values()) < seconds * 1e3 or len(turns[variants[0][0]]) < 10:
        for name, _, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1) / calls)
        if time.perf_counter() - t0 > 120:
            break
    return {k: np.sort(np.asarray(v)) for k, v in turns.items()}


def _line(name, bpp, t, calls=2):
    import numpy as np
    px = SHAPE[0] * SHAPE[1] * SHAPE[2]
    med = float(np.median(t))
    rate = bpp * px / (med * 1e-3)
    print(f"  {name:56s} {bpp:5.1f} B/px  median {med:.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns of {calls} calls)  "
          f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.1f} % of 8 TB/s", flush=True)
    return med


def pixel_loss_only(seconds):
    """The child of --parent: fpcdr_pixel_loss of the package on sys.path, value+grad, on the same seeded tensors."""
    from fpc_diffrend_amd import fit
    colour, rast, ref, _, _ = _tensors()
    t = _take_turns([("parent", 0.0, lambda: fit.pixel_loss_fused(colour, rast, ref))], seconds)["parent"]
    print("PARENT_PIXEL_LOSS " + " ".join(f"{v:.5f}" for v in t), flush=True)


def _child(parent, args):
    env = dict(os.environ, PYTHONPATH=os.path.abspath(parent))
    env.pop("FPCDR_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, cwd=os.path.abspath(parent), check=True,
                         stdout=subprocess.PIPE, timeout=600).stdout.decode()
    return out


def main(commit, seconds, parent):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import robust_ref
    from fpc_diffrend_amd import fit, ops as dr
    assert torch.cuda.is_available(), "needs the GPU"
    B, H, W, C = SHAPE
    colour, rast, ref, mask, face_w = _tensors()
    gs = 1.0 / colour.numel()
    # faster and different is not faster: one image of the batch, cropped, against the torch statement
    crop = lambda t: t[:1, :270, :480].contiguous()
    cc, cr, cf, cm = crop(colour), crop(rast), crop(ref), crop(mask)
    sums, grad = dr.robust_loss_call(cc, cr, cf, 'charbonnier', SCALE, 1.0 / cc.numel(), mask=cm, face_weights=face_w)
    x = cc.clone().requires_grad_(True)
    w, _ = robust_ref.weights(cr[..., 3], cf, cm, face_w, dtype=torch.float32)
    tv = robust_ref.loss_plain(x, cr[..., 3], cf, 'charbonnier', SCALE, weight=w.cuda())
    tv.backward()
    rel = float((grad - x.grad).norm() / x.grad.norm())
    tv = tv.detach()
    print(f"commit {commit}; {B} x {H} x {W} x {C} ({B * H * W / 1e6:.1f} Mpx), c = {SCALE:g}, {T_FACES} face weights; on a 270 x 480 crop "
          f"(Charbonnier, mask, face weights): loss {float(sums[0]) / cc.numel():.6f} torch {float(tv):.6f}, gradient rel-L2 against torch's {rel:.2e}",
          flush=True)
    assert abs(float(sums[0]) / cc.numel() - float(tv)) <= 1e-4 * abs(float(tv)) and rel < 1e-4
    variants = [("fpcdr_pixel_loss value+grad (this build)", 8.0 * C + 17.0, lambda: fit.pixel_loss_fused(colour, rast, ref))]
    for kind in ('l2', 'charbonnier', 'geman_mcclure'):
        for wname, kw, extra in (("", {}, 0.0), (" mask+faces", dict(mask=mask, face_weights=face_w, check_weights=False), 1.0)):
            for gname, want, gb in ((" value", False, 0.0), (" value+grad", True, 4.0 * C)):
                variants.append((f"fpcdr_robust_loss {kind}{wname}{gname}", 4.0 * C + 17.0 + extra + gb,
                                 lambda kind=kind, kw=kw, want=want: dr.robust_loss_call(colour, rast, ref, kind, SCALE, gs, want_grad=want, **kw)))
    # which of the two weights costs what: the mask alone, the face weights alone with the ids drawn per pixel (every lane of a gather
    # in another line of the 120 kB table) and with ids that are constant over 8 x 8 pixels, as a rendered mesh has them
    rast_blocks = rast.clone()
    g = torch.Generator().manual_seed(1)
    blocks = torch.randint(1, T_FACES + 1, (B, H // 8, W // 8), generator=g).float().cuda()
    rast_blocks[..., 3] = torch.where(rast[..., 3] > 0, blocks.repeat_interleave(8, 1).repeat_interleave(8, 2), rast[..., 3])
    variants += [("fpcdr_robust_loss charbonnier mask value+grad", 8.0 * C + 18.0,
                  lambda: dr.robust_loss_call(colour, rast, ref, 'charbonnier', SCALE, gs, mask=mask)),
                 ("fpcdr_robust_loss charbonnier faces value+grad", 8.0 * C + 17.0,
                  lambda: dr.robust_loss_call(colour, rast, ref, 'charbonnier', SCALE, gs, face_weights=face_w, check_weights=False)),
                 ("fpcdr_robust_loss charbonnier faces, ids in 8x8 blocks", 8.0 * C + 17.0,
                  lambda: dr.robust_loss_call(colour, rast_blocks, ref, 'charbonnier', SCALE, gs, face_weights=face_w, check_weights=False)),
                 ("fpcdr_robust_loss charbonnier mask+faces, 8x8 blocks", 8.0 * C + 18.0,
                  lambda: dr.robust_loss_call(colour, rast_blocks, ref, 'charbonnier', SCALE, gs, mask=mask, face_weights=face_w,
                                              check_weights=False))]
    turns = _take_turns(variants, seconds)
    med = {name: _line(name, bpp, turns[name]) for name, bpp, _ in variants}
    base_name, base_bpp = variants[0][0], variants[0][1]
    base = med[base_name]
    if parent:
        out = _child(parent, ["--pixel-loss-only", "--seconds", str(seconds)])
        t = np.sort(np.asarray([float(v) for v in out.split("PARENT_PIXEL_LOSS")[1].split()]))
        base_name = "fpcdr_pixel_loss value+grad (parent build)"
        base = _line(base_name, base_bpp, t)
    print(f"  against {base_name}, time ratio / byte ratio (1.25 allowed for the run-to-run spread of calls this short):")
    for name, bpp, _ in variants[1:]:
        r = (med[name] / base) / (bpp / base_bpp)
        print(f"    {name:56s} time x {med[name] / base:.3f}  bytes x {bpp / base_bpp:.3f}  ratio {r:.3f}{'' if r <= 1.25 else '   ABOVE 1.25'}", flush=True)


def fitter_step(seconds, steps=8):
    """Milliseconds of a whole Fitter step at cfg3's shape, of the package on sys.path: name -> median."""
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg3')
    out = {}
    configs = [("one-pass objective (default)", {}), ("fused_objective=False, L2", dict(fused_objective=False))]
    if hasattr(fit, "pixel_loss_robust"):
        mask = np.random.default_rng(0).integers(0, 256, size=(sc.n_frames, len(sc.cams)) + tuple(sc.resolution), dtype=np.uint8)
        configs.append(("robust: Charbonnier c=10, a mask", dict(robust='charbonnier', robust_scale=SCALE, _masks=mask)))
    for name, kw in configs:
        kw = dict(kw)
        masks = kw.pop("_masks", None)
        s = dataclasses.replace(sc, masks=masks) if masks is not None else sc
        ft = fit.Fitter(s, fit.FitConfig(**kw), device='cuda')
        ft.init_near_truth(0.8)
        for _ in range(3):
            ft.step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            ft.step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = float(np.median(ts))
        print(f"FITTER_STEP {out[name]:.3f} ms  {name}", flush=True)
        del ft
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    secs = float(arg("--seconds", "1.0"))
    if "--pixel-loss-only" in sys.argv:
        pixel_loss_only(secs)
    elif "--fitter-only" in sys.argv:
        fitter_step(secs)
    elif "--fitter" in sys.argv:
        sys.path.insert(0, ROOT)
        print(f"commit {arg('--commit', '(not named)')}; a whole Fitter step at cfg3's shape (32 frames x 9 cameras x 1080 x 1920, 30 k triangles), "
              "host clock around step() + synchronise, median of 8 after 3 warm-up steps:", flush=True)
        fitter_step(secs)
        if arg("--parent", ""):
            print("the parent build:", flush=True)
            print("".join(l + "\n" for l in _child(arg("--parent", ""), ["--fitter-only"]).splitlines() if l.startswith("FITTER_STEP")), flush=True)
    else:
        main(arg("--commit", "(not named)"), secs, arg("--parent", ""))
