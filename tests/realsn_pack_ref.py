"""R3 of csrc/realsn.hip (deqsci_realsn_pack_f32) restated in numpy: the packs of a normalised (C_out, C_in, 3, 3) fp32 weight, in the
order of operations include/deqsci_hip.h states, so that the kernel's outputs can be held to it bit for bit.

    T[a][k] = (G[a][0] g[0][k] + G[a][1] g[1][k]) + G[a][2] g[2][k]          float64, every product and sum rounded by itself,
    U[a][b] = (T[a][0] G[b][0] + T[a][1] G[b][1]) + T[a][2] G[b][2]          G's zeros take part like its other entries
    pack    = float32(U), once, in the kernel's MFMA-lane order

numpy evaluates `x * y + z * w` as separate ufuncs on float64 arrays: no fused multiply-add.  Used by tests/test_realsn_device_gpu.py;
`bound` is the tolerance of that file's comparison with the host packers (_hip.pack_winograd_weights, _hip.pack_winograd44_weights), whose
float64 matrix products sum in an order of their BLAS's choosing."""
import numpy as np

G22 = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=np.float64)
G44 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
               dtype=np.float64)
LAYERS = ((1, 64), (64, 64), (64, 1))


def transposed(w):
    """vjp._transposed: wt[co, ci, ky, kx] = w[ci, co, 2 - ky, 2 - kx]."""
    return np.ascontiguousarray(np.transpose(w, (1, 0, 2, 3))[:, :, ::-1, ::-1])


def transform(w, G):
    """U = G g G^T (C_out, C_in, R, R) float64 of the fp32 weight w, in the stated order."""
    assert w.dtype == np.float32
    g = w.astype(np.float64)
    Ga = G[:, None, None, :]                                             # (a, 1, 1, j)
    T = [None] * 3
    for k in range(3):                                                   # T[..., k][a] over j, left to right
        col = g[None, :, :, :, k]                                        # (1, cout, cin, j)
        T[k] = (Ga[..., 0] * col[..., 0] + Ga[..., 1] * col[..., 1]) + Ga[..., 2] * col[..., 2]      # (a, cout, cin)
    U = np.empty(w.shape[:2] + (G.shape[0], G.shape[0]), dtype=np.float64)
    for b in range(G.shape[0]):
        ub = (T[0] * G[b, 0] + T[1] * G[b, 1]) + T[2] * G[b, 2]          # (a, cout, cin)
        U[:, :, :, b] = np.transpose(ub, (1, 2, 0))
    return U


def magnitude(w, G):
    """|G| |g| |G^T|: what the rounding errors of any float64 evaluation of U are measured against."""
    return np.einsum("aj,oijk,bk->oiab", np.abs(G), np.abs(w.astype(np.float64)), np.abs(G))


def lanes22(U):
    """(64,64,4,4) -> _hip.pack_winograd_weights' order [c][xi][wn][q][i][j][s], cout = 32 wn + 16 j + i, cin = 8 c + 2 q + s."""
    U = np.transpose(U, (2, 3, 0, 1)).reshape(16, 2, 2, 16, 8, 4, 2)    # [xi][wn][j][i][c][q][s]
    return np.ascontiguousarray(np.transpose(U, (4, 0, 1, 5, 3, 2, 6)))


def lanes44(U):
    """(64,64,6,6) -> _hip.pack_winograd44_weights' order [c][sr][sc][rg][cgp][q][i][j][ks]."""
    U = U.reshape(2, 2, 16, 8, 4, 2, 2, 3, 6)                            # [cgp][j][i][c][q][ks][rg][sr][sc]
    return np.ascontiguousarray(np.transpose(U, (3, 7, 8, 6, 0, 4, 2, 1, 5)))


def wide(w):
    """(64,1,3,3) -> _hip.pack_c1_to_64_weights' [tap][cout / 4][cout % 4]."""
    return np.ascontiguousarray(np.transpose(w.reshape(16, 4, 9), (2, 0, 1)))


def narrow(w):
    """(1,64,3,3) -> _hip.pack_c64_to_1_weights' [half][tap][cin % 32]."""
    return np.ascontiguousarray(np.transpose(np.transpose(w, (2, 3, 1, 0)).reshape(9, 2, 32), (1, 0, 2)))


def packs(w):
    """{"pack", "pack44", "pack_t"} of the fp32 weight w (C_out, C_in, 3, 3) as fp32 arrays (pack44: None for an edge layer)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin = w.shape[:2]
    if (cin, cout) == (64, 64):
        return {"pack": lanes22(transform(w, G22)).astype(np.float32), "pack44": lanes44(transform(w, G44)).astype(np.float32),
                "pack_t": lanes22(transform(transposed(w), G22)).astype(np.float32)}
    if (cin, cout) == (1, 64):
        return {"pack": wide(w), "pack44": None, "pack_t": narrow(transposed(w))}
    if (cin, cout) == (64, 1):
        return {"pack": narrow(w), "pack44": None, "pack_t": wide(transposed(w))}
    raise ValueError(f"no pack for a ({cout},{cin},3,3) weight")


def ulp32(x):
    """The spacing of fp32 at |x| (the least subnormal at 0)."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def bound(w):
    """{"pack", "pack44", "pack_t"}: per element of each Winograd pack of the (64,64,3,3) weight w, 16 * 2^-53 * (|G| |g| |G^T|) in the
    pack's order - two float64 evaluations of a 9-term form, each within 8 roundings of the exact value - to which the comparison adds
    one fp32 spacing for the two final roundings."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    c = 16 * 2.0 ** -53
    return {"pack": c * lanes22(magnitude(w, G22)), "pack44": c * lanes44(magnitude(w, G44)), "pack_t": c * lanes22(magnitude(transposed(w), G22))}
