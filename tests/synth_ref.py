"""An independent statement of csrc/synth.hip's Y1 and Y0 for the synth tests.  A helper module, not a test.

The geometry is written out with explicit loops over (i, j, b), straight from include/deqsci_hip.h - nothing of deqsci_amd/synth.py is
used: a row is the ten integers {video_offset, T, Hv, Wv, t0, dt, y0, x0, ds, flags} and the pool one flat uint8 array.  The arithmetic
is fp32 with every product and every sum rounded on its own, b ascending, one division by 255 at the end."""
import numpy as np

FLIP_H, FLIP_V, TRANSPOSE = 1, 2, 4
ORIENTATIONS = tuple(range(8))
F255 = np.float32(255)


def fits(row, H, W, B):
    """All B frames and the four corners of the crop inside the (T,Hv,Wv) video."""
    _, T, Hv, Wv, t0, dt, y0, x0, ds, flags = (int(v) for v in row)
    Hc, Wc = (W, H) if flags & TRANSPOSE else (H, W)
    return dt != 0 and ds >= 1 and 0 <= t0 < T and 0 <= t0 + dt * (B - 1) < T and 0 <= y0 and y0 + ds * (Hc - 1) < Hv \
        and 0 <= x0 and x0 + ds * (Wc - 1) < Wv


def patch_u8(pool, row, H, W, B):
    """The (H,W,B) source bytes of one row.  pool: the flat uint8 array, or its bytes (faster to index one by one)."""
    off, T, Hv, Wv, t0, dt, y0, x0, ds, flags = (int(v) for v in row)
    assert fits(row, H, W, B) and off >= 0 and off + T * Hv * Wv <= len(pool), row
    Hc, Wc = (W, H) if flags & TRANSPOSE else (H, W)
    out = np.empty((H, W, B), np.uint8)
    for i in range(H):
        for j in range(W):
            r, c = (j, i) if flags & TRANSPOSE else (i, j)
            if flags & FLIP_V:
                r = Hc - 1 - r
            if flags & FLIP_H:
                c = Wc - 1 - c
            for b in range(B):
                out[i, j, b] = pool[off + ((t0 + dt * b) * Hv + (y0 + ds * r)) * Wv + (x0 + ds * c)]
    return out


def snapshot(u, mask):
    """-> (gt (H,W,B), meas (H,W)) fp32 of a uint8 block under an fp32 mask (H,W,B)."""
    assert u.dtype == np.uint8 and mask.dtype == np.float32 and u.shape == mask.shape
    uf = u.astype(np.float32)
    s = np.zeros(u.shape[:2], np.float32)
    for b in range(u.shape[2]):
        prod = np.multiply(mask[:, :, b], uf[:, :, b], dtype=np.float32)
        s = np.add(s, prod, dtype=np.float32)
    return np.divide(uf, F255, dtype=np.float32), np.divide(s, F255, dtype=np.float32)


def batch(pool, rows, mask, H, W, B):
    """-> (gt (n,H,W,B), meas (n,H,W)); mask (H,W,B) for all rows or (n,H,W,B)."""
    return snapshots(patches_u8(pool, rows, H, W, B), mask)


def patches_u8(pool, rows, H, W, B):
    """-> (n,H,W,B) uint8: the geometry alone (the slow part: compute it once per set of rows, then any number of masks)"""
    buf = pool.tobytes()
    return np.stack([patch_u8(buf, row, H, W, B) for row in rows]) if len(rows) else np.empty((0, H, W, B), np.uint8)


def snapshots(u, mask):
    gt, meas = np.empty(u.shape, np.float32), np.empty(u.shape[:3], np.float32)
    for k in range(len(u)):
        gt[k], meas[k] = snapshot(u[k], mask[k] if mask.ndim == 4 else mask)
    return gt, meas


def gray(rgb):
    """Y0 in Python integers: (77 R + 150 G + 29 B + 128) >> 8 per triple of a (n,3) uint8 array."""
    return np.array([(77 * int(r) + 150 * int(g) + 29 * int(b) + 128) >> 8 for r, g, b in rgb.reshape(-1, 3)], dtype=np.uint8)
