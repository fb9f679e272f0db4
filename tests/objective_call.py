"""One place for the argument block of fpcdr_objective_fwd when a test only wants the rasteriser's part of the call: the id planes."""
import ctypes

import torch

from helpers import decode_id_planes


def objective_ids(pos, tri, res, bin_lists):
    """fpcdr_objective_fwd, value only, no launch hints, on CPU tensors pos [B,V,4] / tri [T,3] -> triangle + 1 per pixel [B,H,W] int32
    from its id planes (the list kernels of the bin rasteriser; bin_lists: with or without per-bin triangle lists)."""
    from fpc_diffrend_amd import _lib
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd.ops import _ptr, _stream
    lib = _lib.load()
    dev = 'cuda'
    H, W = res
    B, V = pos.shape[:2]
    T = tri.shape[0]
    pos_d, tri_d = pos.to(dev), tri.to(dev)
    adj = dr.antialias_construct_topology_hash(tri_d)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(3)
    uv = torch.rand(V, 2, generator=g).to(dev)
    tri_uv = uv[tri_d.long()].contiguous()
    tex = (torch.rand(16, 16, 1, generator=g) * 0.5).to(dev)
    ref = torch.randint(0, 141, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
    scratch = u8(lib.fpcdr_rasterize_scratch_bytes(B, T))
    sil = u8(B * T)
    idp = u8(lib.fpcdr_idplane_bytes(B, H, W))
    binlist = u8(lib.fpcdr_binlist_bytes(B, H, W)) if bin_lists else None
    occ, cmask = u8(lib.fpcdr_occ_bytes(B, H, W)), u8(lib.fpcdr_objective_cmask_bytes(B, H, W))
    ecol = torch.zeros(4, dtype=torch.float32, device=dev)
    acc = torch.zeros(_lib.LOSS_SLOTS, dtype=torch.float64, device=dev)
    n_rec = B * H * W
    rec = torch.zeros(n_rec, 4, dtype=torch.float32, device=dev)
    color = torch.zeros(n_rec, 1, dtype=torch.float32, device=dev)
    g_aa = torch.zeros(n_rec, 1, dtype=torch.float32, device=dev)
    p = _lib.Objective(pos=_ptr(pos_d), tri=_ptr(tri_d), adj=_ptr(adj), B=B, V=V, T=T, H=H, W=W, scratch=_ptr(scratch), uv=_ptr(uv),
                       uv_tri=_ptr(tri_d), Vt=V, tri_uv=_ptr(tri_uv), tex=_ptr(tex), Ht=16, Wt=16, C=1, boundary_mode=_lib.BOUNDARY['wrap'],
                       ref=_ptr(ref), bg=45.0 / 255.0, color_scale=255.0, grad_scale=1.0 / n_rec, sil=_ptr(sil), idp=_ptr(idp), occ=_ptr(occ),
                       cmask=_ptr(cmask), empty_color=_ptr(ecol), loss_sum=_ptr(acc), grad_pos=None, grad_tex=None, binlist=_ptr(binlist),
                       zero_outputs=1, rec=_ptr(rec), color=_ptr(color), grad_aa=_ptr(g_aa))
    _lib.call("fpcdr_objective_fwd", ctypes.byref(p), _stream())
    torch.cuda.synchronize()
    return decode_id_planes(idp.view(torch.int32).reshape(B, -1), B, H, W)
