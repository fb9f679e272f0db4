"""
Offline multi-camera re-render and numerical comparison of a finished fit -- forward-only consumers of the same
operators.  Host-side mirror of the reference's src/torch/render_multicam.py:95-169
(read result/{i}.obj + texture + pose.json, render every camera, tile 3 x 3) and comparisons.py:54-81
(mean absolute difference over a crop, one CSV line per image).  compare_sequence / compare_result are the same comparison, plus
the heat-map images of comparisons.py:21-50, on the GPU (ops.compare_images -> fpcdr_compare_u8; DESIGN.md 3, "Comparison rule").
overlay_sequence / overlay_result are the pictures of render_result_blended.py -- the re-render laid half-transparent over the capture,
and the mesh's edges drawn over it -- on the GPU (ops.overlay_images -> fpcdr_overlay_u8; DESIGN.md 3, "Overlay rule").
The reference's mp4 / GLFW output is out of scope.
"""
import json
import os

import numpy as np
import torch

from . import camera
from . import ops as dr
from .fit import BACKGROUND, render


def read_result_obj(path):
    """Vertices [V,3] of a result/{i}.obj: the 'v' lines up to the first 'vt' (reference render_multicam.py:121-127)."""
    vertices = []
    with open(path, "r") as f:
        for line in f:
            if line.startswith("v "):
                vertices.extend(float(x) for x in line.strip().split(" ")[1:])
            elif line.startswith("vt "):
                break
    return np.asarray(vertices, dtype=np.float32).reshape(-1, 3)


def read_pose(directory):
    """pose.json of fit.save() (reference fit.py:276-286, read back at render_multicam.py:95-98)."""
    with open(os.path.join(directory, "pose.json"), "r", encoding="utf-8") as f:
        d = json.load(f)
    return np.asarray(d["translation"], dtype=np.float32), np.asarray(d["rotation"], dtype=np.float32)


def read_texture(path):
    """texture.png of fit.save() back to [Ht,Wt,C] float in [0,1] with row 0 at the bottom (it was flipped on save)."""
    from PIL import Image
    img = np.asarray(Image.open(path), dtype=np.float32) / 255.0
    if img.ndim == 2:
        img = img[..., None]
    return np.flip(img, 0).copy()


def make_img(arr, ncols=3):
    """Tile n images [n,H,W,C] into a grid with ncols columns (reference utils.make_img, utils.py:179-190)."""
    n, height, width, nc = arr.shape
    nrows = n // ncols
    assert n == nrows * ncols, "number of images must be a multiple of ncols"
    return arr.reshape(nrows, ncols, height, width, nc).swapaxes(1, 2).reshape(height * nrows, width * ncols, nc)


def _camera_matrices(cams, modelview_offset, dev):
    """(projection [Nc,4,4], modelview [Nc,4,4]) of calib_lookup entries on `dev` (reference render_multicam.py:131-145)."""
    mvps = []
    for c in cams:
        proj = camera.intrinsic_to_projection(c['intr'])
        mv = camera.extrinsic_to_modelview(c['rot'], c['trans_calib']) @ camera.translate(*modelview_offset)
        mvps.append((proj, mv))
    proj = torch.tensor(np.stack([p for p, _ in mvps]), dtype=torch.float32, device=dev)
    t_mv = torch.tensor(np.stack([m for _, m in mvps]), dtype=torch.float32, device=dev)
    return proj, t_mv


def _multicam_mvp(proj, t_mv, pose):
    """Model-view-projection [Nc,4,4] with the optional rigid head pose (t [3], q [4]) applied (render_multicam.py:146-150)."""
    if pose is not None:
        t, q = (torch.as_tensor(a, dtype=torch.float32, device=proj.device) for a in pose)
        t_mv = torch.matmul(camera.rigid_grad(t, camera.unitquat_to_rotmat(q))[None], t_mv)
    return torch.matmul(proj, t_mv)


@torch.no_grad()
def render_multicam(glctx, vertices, pos_idx, uv, uv_idx, tex, cams, resolution, pose=None, modelview_offset=(0.0, 0.0, 0.0)):
    """All cameras of the rig for one mesh: [Nc,H,W,C] in 0..255, top row first (reference render_multicam.py:131-158).

    vertices [V,3] tensor; cams: calib_lookup entries; pose: optional (t [3], q [4]) rigid head pose applied like
    `reproduce_pose` (render_multicam.py:146-150).  One batched launch per operator instead of one render per camera."""
    dev = vertices.device
    mvp = _multicam_mvp(*_camera_matrices(cams, modelview_offset, dev), pose)
    colour = render(glctx, mvp, vertices[None], pos_idx, uv, uv_idx, tex, resolution, False, 0) * 255.0
    return torch.flip(colour, dims=[1])      # row 0 = bottom in the raster -> top row first on disk


def mean_abs_diff(img, ref, rows=(200, 1401), cols=(100, 1100)):
    """(image mean, per-row means) of |img - ref| over a crop (reference comparisons.py:66-75: rows 200..1400 inclusive,
    columns 100..1099, integer arithmetic).  The crop is clipped to the image."""
    a = np.asarray(img).astype(np.int32)
    b = np.asarray(ref).astype(np.int32)
    r0, r1 = max(rows[0], 0), min(rows[1], a.shape[0])
    c0, c1 = max(cols[0], 0), min(cols[1], a.shape[1])
    row_means = np.abs(a[r0:r1, c0:c1] - b[r0:r1, c0:c1]).reshape(r1 - r0, -1).mean(axis=1)
    return float(row_means.mean()), row_means


def _csv_line(m, rows):
    """One image's line of numerical_clip.csv: 'image mean, row means...' (reference comparisons.py:79)."""
    return f"{m}, {', '.join(str(x) for x in rows)}\n"


def _csv_last_line(means):
    """The file's last line, without a line end: the mean of the image means (reference comparisons.py:80)."""
    return str(float(np.mean(means)))


def compare_sequence_numerical(inferred, references, csv_path, **crop):
    """One CSV line per image 'mean, row means...' and the mean of means last (reference comparisons.py:56-80).
    inferred / references: sequences of arrays.  Returns the list of image means."""
    os.makedirs(os.path.dirname(os.path.abspath(csv_path)), exist_ok=True)
    means = []
    with open(csv_path, "w") as f:
        for img, ref in zip(inferred, references):
            m, rows = mean_abs_diff(img, ref, **crop)
            means.append(m)
            f.write(_csv_line(m, rows))
        f.write(_csv_last_line(means))
    return means


def _load_result(result_dir, sc, dev, reproduce_pose, frames=None, cams=None):
    """A directory written by Fitter.save() on `dev`, with what the reference re-reads from the take taken from sc.  Returns
      mesh    (pos_idx, uv, uv_idx, tex), in the order render_multicam and fit.render_from_clip take them
      pose    the saved (translations [F,3], rotations [F,4]) of pose.json, or None with reproduce_pose=False (_pose_of takes a frame's)
      frames  the frame numbers as a list (default: every {i}.obj of the result)
      cams    indices into sc.cams as a list (default: all)"""
    mesh = (torch.tensor(sc.pos_idx, dtype=torch.int32, device=dev), torch.tensor(sc.uv, dtype=torch.float32, device=dev),
            torch.tensor(sc.uv_idx, dtype=torch.int32, device=dev),
            torch.tensor(read_texture(os.path.join(result_dir, "texture.png")), dtype=torch.float32, device=dev))
    pose = read_pose(result_dir) if reproduce_pose else None
    if frames is None:
        frames = range(len([f for f in os.listdir(result_dir) if f.endswith(".obj") and f[:-4].isdigit()]))
    return mesh, pose, list(frames), list(range(len(sc.cams))) if cams is None else [int(c) for c in cams]


def _pose_of(pose, i):
    return (pose[0][i], pose[1][i]) if pose is not None else None


@torch.no_grad()
def rerender_result(result_dir, sc, device='cuda', frames=None, reproduce_pose=True, ncols=3):
    """Re-render a directory written by Fitter.save(): yields (frame index, grid image uint8 [3H,3W,C]).
    sc supplies what the reference re-reads from the take (index buffers, uv, cameras, resolution)."""
    dev = torch.device(device)
    glctx = dr.RasterizeGLContext(device=dev)
    mesh, pose, frames, _ = _load_result(result_dir, sc, dev, reproduce_pose, frames)
    for i in frames:
        verts = torch.tensor(read_result_obj(os.path.join(result_dir, f"{i}.obj")), device=dev)
        imgs = render_multicam(glctx, verts, *mesh, sc.cams, sc.resolution, pose=_pose_of(pose, i), modelview_offset=(0.0, 170.0, 0.0))
        grid = make_img(imgs.cpu().numpy(), ncols=ncols)
        yield i, np.clip(np.rint(grid), 0, 255).astype(np.uint8)


# ---- the same comparison on the GPU ------------------------------------------------------------------------------------------------
def _crop(H, W, rows, cols):
    """The crop clipped to the image, as mean_abs_diff clips it; an empty one has no mean."""
    r0, r1 = max(rows[0], 0), min(rows[1], H)
    c0, c1 = max(cols[0], 0), min(cols[1], W)
    if r0 >= r1 or c0 >= c1:
        raise ValueError(f"the crop rows {tuple(rows)}, cols {tuple(cols)} is empty on a {H} x {W} image")
    return r0, r1, c0, c1


def _means_of_row_sums(sums, crop):
    """(image mean, per-row means) from one image's integer row sums [H] over the crop's columns: the second output of mean_abs_diff
    is np.mean of an int32 row, i.e. exactly float64(sum) / columns, and the first is the same .mean() of the same float64 array."""
    r0, r1, c0, c1 = crop
    row_means = np.asarray(sums[r0:r1]).astype(np.float64) / (c1 - c0)
    return float(row_means.mean()), row_means


def _gpu(device):
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError("the comparison runs on an MI355X (device='cuda'): the HIP path has no CPU fallback")
    return dev


def _pair_batches(inferred, references, batch, dev):
    """(number of the first pair, inferred [n,H,W], references [n,H,W]) on `dev`, `batch` pairs at a time."""
    for b0 in range(0, len(inferred), batch):
        yield (b0, torch.from_numpy(np.stack([np.asarray(a) for a in inferred[b0:b0 + batch]])).to(dev),
               torch.from_numpy(np.stack([np.asarray(a) for a in references[b0:b0 + batch]])).to(dev))


def compare_sequence(inferred, references, out_dir, colour=True, heat=True, rows=(200, 1401), cols=(100, 1100), device='cuda', batch=16):
    """compareSequenceNumerical and (heat=True) the heat-map images of compareSequence (reference comparisons.py:21-80) for a sequence
    of image pairs, on the GPU: writes out_dir/numerical_clip.csv -- the text compare_sequence_numerical writes -- and
    out_dir/colcomp_{i}.png (colour=False: the grey map).  inferred / references: sequences of uint8 arrays [H,W] of one shape, top row
    first; they are uploaded `batch` pairs at a time and go through ops.compare_images.  Returns the list of image means."""
    dev = _gpu(device)
    assert len(inferred) == len(references), "as many inferred images as references"
    os.makedirs(out_dir, exist_ok=True)
    mode = ('colour' if colour else 'grey') if heat else None
    means = []
    with open(os.path.join(out_dir, "numerical_clip.csv"), "w") as f:
        for b0, img, ref in _pair_batches(inferred, references, batch, dev):
            crop = _crop(img.shape[1], img.shape[2], rows, cols)
            maps, sums = dr.compare_images(img, ref, mode=mode, cols=cols)
            sums = sums.cpu().numpy()
            maps = maps.cpu().numpy() if heat else None
            for k in range(sums.shape[0]):
                m, row_means = _means_of_row_sums(sums[k], crop)
                means.append(m)
                f.write(_csv_line(m, row_means))
                if heat:
                    _write_png(os.path.join(out_dir, f"colcomp_{b0 + k}.png"), maps[k])
        f.write(_csv_last_line(means))
    return means


def _write_png(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path)


def take_references(imdir):
    """`references` of compare_result for a take on disk in the layout scene.from_take reads: frame -> [Nc,H,W] uint8, top row first,
    unclipped (data.load_raw_image), the camera directories in sorted order as in from_take."""
    from . import data
    cams = sorted(os.listdir(imdir))
    _, digits = data.assert_num_frames(cams, imdir)
    return lambda frame: np.stack([data.load_raw_image(os.path.join(imdir, c, f"{c}_{frame:0{digits}d}.tif")) for c in cams])


def _frame_batches(result_dir, sc, loaded, references, batch_frames, dev, what):
    """The re-renders of a saved result (loaded = _load_result's tuple) beside their captures, its cameras of `batch_frames` frames
    at a time.  Yields (the chunk's place b0 in the frame list, its frame numbers, colour [n,H,W,1] float in [0,1] with the background
    composited, contiguous, rast, rast_db, captures uint8 [n,H,W] on `dev`), n = frames x cameras, every raster with row 0 at the
    bottom.  The colour is fit.render_from_clip's unfused non-mip operator sequence with the rasteriser's second output kept.
    what: the caller's noun for the one-channel check's message."""
    glctx = dr.RasterizeGLContext(device=dev)
    (pos_idx, uv, uv_idx, tex), pose, frames, cams = loaded
    proj, t_mv = _camera_matrices([sc.cams[c] for c in cams], (0.0, 170.0, 0.0), dev)
    shape = (len(cams),) + tuple(sc.resolution)
    for b0 in range(0, len(frames), batch_frames):
        chunk = frames[b0:b0 + batch_frames]
        clip, refs = [], []
        for i in chunk:
            verts = torch.tensor(read_result_obj(os.path.join(result_dir, f"{i}.obj")), device=dev)
            # per frame exactly the matrices and the transform of render_multicam: the same clip-space positions, bit for bit
            clip.append(camera.transform_clip(_multicam_mvp(proj, t_mv, _pose_of(pose, i)), verts[None]))
            r = np.asarray(references(i) if callable(references) else references[i])
            if r.dtype != np.uint8 or r.shape != shape:
                raise ValueError(f"references of frame {i}: expected uint8 {shape}, got {r.dtype} {r.shape}")
            refs.append(r)
        pos_clip = torch.cat(clip)
        rast, rast_db = dr.rasterize(glctx, pos_clip, pos_idx, resolution=(sc.resolution[0], sc.resolution[1]))
        texc, _ = dr.interpolate(uv[None, ...], rast, uv_idx)
        colour_img = dr.antialias(dr.texture(tex[None, ...], texc, filter_mode='linear'), rast, pos_clip, pos_idx)
        if colour_img.shape[-1] != 1:
            raise ValueError(f"the {what} is of one-channel images (the texture has {colour_img.shape[-1]} channels)")
        colour_img = torch.where(rast[..., 3:] > 0, colour_img, torch.tensor(BACKGROUND, device=dev))
        yield b0, chunk, colour_img.contiguous(), rast, rast_db, torch.from_numpy(np.concatenate(refs)).to(dev)


@torch.no_grad()
def compare_result(result_dir, sc, references, out_dir, cams=None, frames=None, reproduce_pose=True, colour=True, heat=True,
                   batch_frames=4, device='cuda', **crop):
    """Re-render a directory written by Fitter.save() and compare it with the captures without the images leaving the GPU: the chosen
    cameras of `batch_frames` frames are rendered at once, and the render's [0,1] output goes straight into ops.compare_images
    (scale=255, flip_rows=True: the raster has row 0 at the bottom, the captures their top row first) -- what reaches the host is the
    row sums and, with heat=True, the heat maps.

      references  uint8 [F,Nc,H,W] indexed by frame number, top row first, or a callable frame -> [Nc,H,W] (take_references for a take
                  on disk); camera axis in the order of `cams`
      cams        indices into sc.cams (default: all); frames: frame numbers (default: every {i}.obj of the result)
      crop        rows=, cols= as mean_abs_diff

    Writes out_dir/numerical_clip_<cam>.csv per camera (<cam> = its index in sc.cams; one line per frame, in the format of
    compare_sequence_numerical) and out_dir/colcomp_<cam>_<frame>.png.  Returns the image means as a float64 array [frames, cams]."""
    dev = _gpu(device)
    rows, cols = crop.pop('rows', (200, 1401)), crop.pop('cols', (100, 1100))
    if crop:
        raise TypeError(f"unknown arguments {sorted(crop)}")
    H, W = sc.resolution
    box = _crop(H, W, rows, cols)
    loaded = _load_result(result_dir, sc, dev, reproduce_pose, frames, cams)
    _, _, frames, cams = loaded
    Nc = len(cams)
    os.makedirs(out_dir, exist_ok=True)
    mode = ('colour' if colour else 'grey') if heat else None
    means = np.empty((len(frames), Nc), dtype=np.float64)
    lines = [[] for _ in cams]
    for b0, chunk, colour_img, _, _, ref in _frame_batches(result_dir, sc, loaded, references, batch_frames, dev, 'comparison'):
        maps, sums = dr.compare_images(colour_img, ref, mode=mode, cols=cols, scale=255.0, flip_rows=True)
        sums = sums.cpu().numpy().reshape(len(chunk), Nc, H)
        maps = maps.cpu().numpy().reshape(len(chunk), Nc, H, W, 3) if heat else None
        for k, i in enumerate(chunk):
            for j, c in enumerate(cams):
                m, row_means = _means_of_row_sums(sums[k, j], box)
                means[b0 + k, j] = m
                lines[j].append(_csv_line(m, row_means))
                if heat:
                    _write_png(os.path.join(out_dir, f"colcomp_{c}_{i}.png"), maps[k, j])
    for j, c in enumerate(cams):
        with open(os.path.join(out_dir, f"numerical_clip_{c}.csv"), "w") as f:
            f.writelines(lines[j])
            f.write(_csv_last_line(means[:, j]))
    return means


# ---- the re-render over the capture ------------------------------------------------------------------------------------------------
def overlay_sequence(inferred, references, out_dir, weight=0.5, device='cuda', batch=16):
    """The blended images of the reference's render_result_blended.py:149-154 -- np.clip(np.rint(ref * 0.5 + img * 0.5), 0, 255) at the
    default weight -- for a sequence of image pairs, on the GPU: writes out_dir/overlay_{i}.png (grey, three equal channels).
    inferred / references: sequences of uint8 arrays [H,W] of one shape, top row first; they are uploaded `batch` pairs at a time and go
    through ops.overlay_images."""
    dev = _gpu(device)
    assert len(inferred) == len(references), "as many inferred images as references"
    os.makedirs(out_dir, exist_ok=True)
    for b0, img, ref in _pair_batches(inferred, references, batch, dev):
        out = dr.overlay_images(img, ref, weight=weight).cpu().numpy()
        for k in range(out.shape[0]):
            _write_png(os.path.join(out_dir, f"overlay_{b0 + k}.png"), out[k])


@torch.no_grad()
def overlay_result(result_dir, sc, references, out_dir, cams=None, frames=None, reproduce_pose=True, wireframe=True,
                   wire_colour=(0, 255, 0), half_width=0.5, weight=0.5, outside='capture', batch_frames=4, device='cuda'):
    """Re-render a directory written by Fitter.save() and lay it over the captures, with the mesh's edges drawn (wireframe=True), without
    a float image leaving the GPU: the picture to look at first to see whether a fit sits on the face (the reference's
    render_result_blended.py; its wireframe variant needs a painted texture, this one draws the edges from the rasteriser's
    barycentrics and their screen derivatives).  Arguments and batching as compare_result; every frame's matrices and clip-space
    positions are formed the same way and the colour by the same operators (_frame_batches), so it equals compare_result's bit for bit.

      references   uint8 [F,Nc,H,W] indexed by frame number, top row first, or a callable frame -> [Nc,H,W]
      wire_colour  (r, g, b) bytes of the lines; half_width: half a line's width in pixels (a line is drawn from both sides of an edge)
      weight       the render's share of the blend; outside: 'capture' shows the capture unchanged off the mesh, 'render' blends the
                   background colour in as the reference does

    Writes out_dir/overlay_<cam>_<frame>.png (<cam> = the camera's index in sc.cams)."""
    dev = _gpu(device)
    loaded = _load_result(result_dir, sc, dev, reproduce_pose, frames, cams)
    cams = loaded[3]
    Nc = len(cams)
    H, W = sc.resolution
    os.makedirs(out_dir, exist_ok=True)
    for _, chunk, colour_img, rast, rast_db, ref in _frame_batches(result_dir, sc, loaded, references, batch_frames, dev, 'overlay'):
        out = dr.overlay_images(colour_img, ref, rast=rast.contiguous(), rast_db=rast_db.contiguous(), weight=weight, outside=outside,
                                wire=tuple(wire_colour) if wireframe else None, half_width=half_width, scale=255.0, flip_rows=True)
        out = out.cpu().numpy().reshape(len(chunk), Nc, H, W, 3)
        for k, i in enumerate(chunk):
            for j, c in enumerate(cams):
                _write_png(os.path.join(out_dir, f"overlay_{c}_{i}.png"), out[k, j])
