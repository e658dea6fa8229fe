"""fp64 reference of the low-resolution pyramid tail (gw_depth_amd/csrc/pyrtail.hip, ops._PyramidTailFn), plain torch on the CPU.

The identity: a 3x3 convolution (zero padding 1) over an align-corners bilinear up-sampling of y equals, tap by tap, the up-sampling
of the channel products W_tap . y read one pixel over:

    conv3x3(up(y))(p) = sum_tap [p + tap inside the map] * up(W_tap . y)(p + tap)

The resize's weights are the ones the kernels (and torch's own fp32 up-sampling) use: the source coordinate dst * (h - 1) / (H - 1)
is formed in fp32, its integer part picks the two taps, its fp32 fraction l and 1 - l weigh them.  From there on everything is fp64.
"""
import numpy as np
import torch


def resize_matrix(h, H):
    """U (H, h) fp64: row o holds the two weights with which output coordinate o reads the h source coordinates."""
    U = torch.zeros(H, h, dtype=torch.float64)
    scale = np.float32(h - 1) / np.float32(H - 1) if H > 1 else np.float32(0.0)
    for o in range(H):
        f = np.float32(scale * np.float32(o))
        i0 = int(f)
        i1 = i0 + (1 if i0 < h - 1 else 0)
        l = np.float32(f - np.float32(i0))
        U[o, i0] += float(np.float32(1.0) - l)
        U[o, i1] += float(l)
    return U


def _shift_into(dst, src, ty, tx):
    """dst[:, y, x] += src[:, y + ty, x + tx] wherever (y + ty, x + tx) lies inside the map (the convolution's zero padding)."""
    H, W = dst.shape[1], dst.shape[2]
    y0, y1, x0, x1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
    if y1 > y0 and x1 > x0:
        dst[:, y0:y1, x0:x1] += src[:, y0 + ty:y1 + ty, x0 + tx:x1 + tx]
    return dst


def tail_z(part, Zs):
    """part (B,H,W,N), Zs[k] (B,h,w,9,N), any float type -> (z, S) fp64: the sum the forward kernel forms, and the sum of the absolute
    values of its terms (for the summation bound)."""
    B, H, W, N = part.shape
    z, S = part.double().clone(), part.double().abs()
    for Z in Zs:
        h, w = Z.shape[1], Z.shape[2]
        Uy, Ux = resize_matrix(h, H), resize_matrix(w, W)
        Zd = Z.double()
        up = torch.einsum("Yh,Xw,bhwtn->bYXtn", Uy, Ux, Zd)
        upa = torch.einsum("Yh,Xw,bhwtn->bYXtn", Uy, Ux, Zd.abs())
        for t in range(9):
            ty, tx = t // 3 - 1, t % 3 - 1
            _shift_into(z, up[:, :, :, t], ty, tx)
            _shift_into(S, upa[:, :, :, t], ty, tx)
    return z, S


def tail_G(gz, h, w):
    """gz (B,H,W,N) -> (G, S, n): G (B,h,w,9,N) fp64 = the gradient of a product map, S the sum of |terms|, n (h,w,9) the number of
    terms of each element (its footprint)."""
    B, H, W, N = gz.shape
    Uy, Ux = resize_matrix(h, H), resize_matrix(w, W)
    g = gz.double()
    G = torch.zeros(B, h, w, 9, N, dtype=torch.float64)
    S = torch.zeros_like(G)
    n = torch.zeros(h, w, 9, dtype=torch.float64)
    ones = torch.ones(1, H, W, 1, dtype=torch.float64)
    for t in range(9):
        ty, tx = t // 3 - 1, t % 3 - 1
        # gs[y', x'] = gz[y' - ty, x' - tx]: the pixel whose tap (ty, tx) reads source pixel (y', x')
        gs = _shift_into(torch.zeros_like(g), g, -ty, -tx)
        G[:, :, :, t] = torch.einsum("Yh,Xw,bYXn->bhwn", Uy, Ux, gs)
        S[:, :, :, t] = torch.einsum("Yh,Xw,bYXn->bhwn", Uy, Ux, gs.abs())
        inside = _shift_into(torch.zeros_like(ones), ones, -ty, -tx)
        n[:, :, t] = torch.einsum("Yh,Xw,bYXn->bhwn", (Uy > 0).double(), (Ux > 0).double(), inside)[0, :, :, 0]
    return G, S, n


def up_ac(y, H, W):
    """(B,h,w,C) -> (B,H,W,C): the align-corners bilinear resize with the weights above (differentiable)."""
    Uy, Ux = resize_matrix(y.shape[1], H).to(y.dtype), resize_matrix(y.shape[2], W).to(y.dtype)
    return torch.einsum("Yh,Xw,bhwc->bYXc", Uy, Ux, y)


def conv3x3(x, w):
    """x (B,H,W,C), w (N,3,3,C) -> (B,H,W,N), zero padding 1."""
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)


def tail_direct(x, ys, w):
    """conv3x3([x | up(y_1) | ... ], w): today's formulation."""
    H, W = x.shape[1], x.shape[2]
    return conv3x3(torch.cat([x] + [up_ac(y, H, W) for y in ys], dim=-1), w)


def tail_decomposed(x, ys, w, nlow):
    """The same map with the first nlow branches convolved at their own resolution (differentiable; what ops._PyramidTailFn runs)."""
    B, H, W, C2 = x.shape
    N = w.shape[0]
    w_hi = torch.cat([w[..., :C2], w[..., (1 + nlow) * C2:]], dim=-1)
    z = conv3x3(torch.cat([x] + [up_ac(y, H, W) for y in ys[nlow:]], dim=-1), w_hi)
    for k, y in enumerate(ys[:nlow]):
        wl = w[..., (k + 1) * C2:(k + 2) * C2].permute(1, 2, 0, 3).reshape(9 * N, C2)
        Z = (y @ wl.t()).reshape(B, y.shape[1], y.shape[2], 9, N)
        up = torch.einsum("Yh,Xw,bhwtn->bYXtn", resize_matrix(y.shape[1], H).to(y.dtype), resize_matrix(y.shape[2], W).to(y.dtype), Z)
        for t in range(9):
            ty, tx = t // 3 - 1, t % 3 - 1
            pad = torch.nn.functional.pad(up[:, :, :, t], (0, 0, 1, 1, 1, 1))
            z = z + pad[:, 1 + ty:1 + ty + H, 1 + tx:1 + tx + W]
    return z
