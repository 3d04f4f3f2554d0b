"""What a NaN or an Inf in a convolution's input must do to its output, stated once for tests/test_nonfinite_host.py (the helper against
float64) and tests/test_nonfinite_gpu.py (the kernels against both).  A helper module, not a test.

The REFERENCE of an operation is float64 torch on the same poisoned operands: conv2d(double, padding=1) + bias, then torch.relu - which
propagates NaN and maps -Inf to 0 -, pixel_unshuffle / pixel_shuffle around FFDNet's edge layers, and for a masked layer a SELECT
(mask ? v : 0, as torch's ReLU backward is: a NaN under a cleared bit is 0).

reach(poison, H, W, tile) is where a kernel MAY differ from its own clean launch: per image, the union of the kernel's output tiles
(th x tw, aligned at the image's origin - every kernel here starts its tiling at pixel (0, 0)) that intersect the clipped 3 x 3 dilation
of the poisoned pixels.  A kernel that computes every output pixel from its own 3 x 3 window has a 1 x 1 tile and its reach is the
dilation itself; a Winograd kernel computes a tile of outputs from shared transformed sums, where Inf - Inf or 0 * NaN may turn the whole
tile NaN.  Outside reach, and in every other image, the poisoned launch must give the clean launch's bits.

Tile sizes, read out of the kernels (CASES below names them beside each case):
  1 x 1  csrc/ffdnet_edges.hip (conv_c1_to_64_kernel, ffdnet_head_kernel, ffdnet_head_mfma_kernel, edge_tail_kernel: an accumulator per
         output position; the MFMA head's positions are matrix columns, which do not mix), csrc/conv_s16.hip (conv_s16_kernel, head_s16_kernel,
         tail_s16_kernel: direct sums, pixels are matrix rows / columns), csrc/jacobian.hip's and vjp's masked heads
  1 x 2  csrc/conv_w16.hip: Winograd F(2,3) along x only, a lane owns a column PAIR
  2 x 2  csrc/winograd.hip: F(2x2,3x3), `oy = 2 * (...)`, `ox = 2 * (...)`
  4 x 4  csrc/winograd44.hip: F(4x4,3x3), `oy = OUT_ROWS * by + 4 * (...)`, `ox = OUT_COLS * bx + 4 * (...)`
FFDNet's head works at half resolution (a full-resolution pixel maps to (r // 2, c // 2) before the dilation); its tail's every
half-resolution output position is a 2 x 2 block of full-resolution pixels."""
import torch
import torch.nn.functional as Fn

POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
CHANNELS = (0, 31, 63)


# ----------------------------------------------------------------------------- the float64 reference
def conv_ref(x, w, bias=None, relu=False, mask=None):
    """relu(conv2d(x, w, padding=1) + bias) in float64 on the CPU; mask (bool, the output's shape): the select mask ? v : 0 instead."""
    y = Fn.conv2d(x.detach().double().cpu(), w.detach().double().cpu(), None if bias is None else bias.detach().double().cpu(), padding=1)
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = torch.where(mask.cpu(), y, torch.zeros((), dtype=torch.float64))
    return y


def ffdnet_head_ref(x, sigma, w, relu=True, mask=None, with_sigma=True):
    """FFDNet's first layer: cat(sigma map, pixel_unshuffle(x, 2)) -> conv3x3 [-> ReLU]; sigma (n,) or (1,).  with_sigma=False: the
    linearised layer (image channels 1..4 only: w is then (64,4,3,3))."""
    xd = Fn.pixel_unshuffle(x.detach().double().cpu(), 2)
    if with_sigma:
        n, _, H, W = xd.shape
        xd = torch.cat((sigma.detach().double().cpu().reshape(-1, 1, 1, 1).expand(n, 1, H, W), xd), 1)
    return conv_ref(xd, w, None, relu, mask)


def tail_ref(h, w, in_bias=None, shuffle=False):
    """The last layer on h' = h, or relu(h + in_bias) when in_bias is given; shuffle: FFDNet's pixel_shuffle(2) behind it."""
    hd = h.detach().double().cpu()
    if in_bias is not None:
        hd = torch.relu(hd + in_bias.detach().double().cpu().view(1, -1, 1, 1))
    y = conv_ref(hd, w)
    return Fn.pixel_shuffle(y, 2) if shuffle else y


def stack_ref(x, layers):
    """A run of layers [(w, bias or None, relu)] in float64."""
    h = x
    for w, b, relu in layers:
        h = conv_ref(h, w, b, relu)
    return h


def pack_mask(bits):
    """bool (n,64,H,W) -> the int64 (n,H,W) words of relu_mask_pack: bit c = channel c."""
    out = torch.zeros(bits.shape[0], bits.shape[2], bits.shape[3], dtype=torch.int64, device=bits.device)
    for c in range(64):
        word = (1 << c) if c < 63 else -(1 << 63)
        out |= bits[:, c].to(torch.int64) * word
    return out


# ----------------------------------------------------------------------------- reach
def dilate(p):
    """bool (n,H,W) -> its 3 x 3 dilation, clipped at the image's border (the convolution's zero padding holds no poison)."""
    return Fn.max_pool2d(p.float().unsqueeze(1), 3, stride=1, padding=1).squeeze(1) > 0


def tiles_of(hit, tile):
    """bool (n,H,W) -> the union of the th x tw tiles (aligned at the origin, clipped at the image) that hold a hit."""
    th, tw = tile
    n, H, W = hit.shape
    t = Fn.max_pool2d(hit.float().unsqueeze(1), (th, tw), stride=(th, tw), ceil_mode=True)           # one value per tile
    return t.repeat_interleave(th, 2).repeat_interleave(tw, 3)[:, 0, :H, :W] > 0


def reach(poison, H, W, tile, layers=1):
    """poison: bool (n,H,W), a poisoned input pixel in ANY channel -> bool (n,H,W), the output pixels a kernel of output tile `tile` may
    change; layers > 1: a run of that many launches of the kernel (every changed pixel is a poison of the next layer)."""
    assert poison.dtype == torch.bool and tuple(poison.shape[1:]) == (H, W)
    r = poison.cpu()
    for _ in range(layers):
        r = tiles_of(dilate(r), tile)
    return r


def reach_head(poison_full, H, W, tile):
    """FFDNet's first layer: poison (n,2H,2W) at full resolution -> reach (n,H,W) at half resolution."""
    assert tuple(poison_full.shape[1:]) == (2 * H, 2 * W)
    half = Fn.max_pool2d(poison_full.cpu().float().unsqueeze(1), 2).squeeze(1) > 0
    return reach(half, H, W, tile)


def reach_tail(poison_half, H, W, tile):
    """FFDNet's last layer: poison (n,H,W) at half resolution -> reach (n,2H,2W): every half-resolution position is a 2 x 2 block."""
    return reach(poison_half, H, W, tile).repeat_interleave(2, 1).repeat_interleave(2, 2)


def positions(n, H, W, row_seams=(), col_seams=()):
    """The poisoned positions (image, row, column) of a case, one per run: the four corners of image 0, the last pixel of image 0 and the
    first of image 1 (the seam between two images), and one pixel on each side of every seam of the kernel's tiling inside the shape -
    row seams at a middle column that is itself no seam, column seams at such a row."""
    assert n >= 2
    seams_r = sorted({s for s in row_seams if 0 < s < H})
    seams_c = sorted({s for s in col_seams if 0 < s < W})
    mid_r = next(r for r in range(H // 2, H) if r not in seams_r and r + 1 not in seams_r)
    mid_c = next(c for c in range(W // 2, W) if c not in seams_c and c + 1 not in seams_c)
    pos = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (1, 0, 0)]
    for s in seams_r:
        pos += [(0, s - 1, mid_c), (0, s, mid_c)]
    for s in seams_c:
        pos += [(0, mid_r, s - 1), (0, mid_r, s)]
    return list(dict.fromkeys(pos))


# ----------------------------------------------------------------------------- the GPU table
# name -> (n, H, W) of the grid the kernel tiles (FFDNet's edge layers: the half-resolution grid), the output tile (th, tw), the seams of
# the kernel's tiling inside the shape (rows, columns: Winograd tile, block tile = workgroup tile), and `res`: where the poison goes in
# ("same": on that grid; "full": FFDNet's head, the image is (2H, 2W)) and what comes out ("same" / "full": the tail's pixel shuffle).
# Shapes: two images, ragged against every tile in both directions, odd width.
CASES = {
    # csrc/winograd.hip: Winograd tile 2 x 2, block tile (one persistent workgroup's unit) 8 x 8 Winograd tiles = 16 x 16
    "f22": dict(shape=(2, 19, 35), tile=(2, 2), rows=(2, 16, 18), cols=(2, 16, 32, 34), src="same", dst="same"),
    # csrc/winograd44.hip: Winograd tile 4 x 4, block tile 4 x 8 Winograd tiles = 16 x 32; blk32 blocks of 32 columns
    "f44": dict(shape=(2, 19, 35), tile=(4, 4), rows=(4, 16), cols=(4, 32), src="same", dst="same"),
    # csrc/conv_s16.hip conv_s16_kernel: direct, OUT_ROWS x OUT_COLS = 16 x 32 block tile
    "s16": dict(shape=(2, 19, 35), tile=(1, 1), rows=(16,), cols=(32,), src="same", dst="same"),
    # csrc/conv_w16.hip: F(2,3) along x on column pairs, block tile 8 x 64 (p32 blocks of 64 columns)
    "w16": dict(shape=(2, 10, 67), tile=(1, 2), rows=(8,), cols=(2, 64, 66), src="same", dst="same"),
    # csrc/ffdnet_edges.hip conv_c1_to_64_kernel: H1_T = 32 square tiles, 16 positions per trip
    "c1_to_64": dict(shape=(2, 34, 35), tile=(1, 1), rows=(32,), cols=(16, 32), src="same", dst="same"),
    # csrc/ffdnet_edges.hip ffdnet_head_kernel<16> (the small-launch form): 16 x 16 half-resolution positions
    "head_valu": dict(shape=(2, 18, 19), tile=(1, 1), rows=(16,), cols=(16,), src="full", dst="same"),
    # csrc/ffdnet_edges.hip ffdnet_head_mfma_kernel (launches of >= 2 tiles per CU): 32 x 32 positions, groups of 16 columns
    "head_mfma": dict(shape=(130, 128, 128), tile=(1, 1), rows=(32,), cols=(16, 32), src="full", dst="same"),
    # csrc/conv_s16.hip head_s16_kernel: HS_H x HS_W = 8 x 32 positions
    "head_s16": dict(shape=(2, 10, 35), tile=(1, 1), rows=(8,), cols=(32,), src="full", dst="same"),
    # csrc/ffdnet_edges.hip edge_tail_kernel: TT_H x TT_W = 8 x 32 positions (FFDNet: each a 2 x 2 block of the output)
    "tail_valu_ffdnet": dict(shape=(2, 10, 35), tile=(1, 1), rows=(8,), cols=(32,), src="same", dst="full"),
    "tail_valu_c1": dict(shape=(2, 10, 35), tile=(1, 1), rows=(8,), cols=(32,), src="same", dst="same"),
    # csrc/conv_s16.hip tail_s16_kernel: TL_H x TL_W = 8 x 32 positions, halo pixels in blocks of 32; the p32 input in blocks of 64 columns
    "tail_s16_ffdnet": dict(shape=(2, 10, 67), tile=(1, 1), rows=(8,), cols=(32, 64), src="same", dst="full"),
    "tail_s16_c1": dict(shape=(2, 10, 67), tile=(1, 1), rows=(8,), cols=(32, 64), src="same", dst="same"),
}


def case_positions(name):
    c = CASES[name]
    n, H, W = c["shape"]
    if name == "head_mfma":                # one poison set on the big launch: the corner where a row seam and a column seam of the tiling meet
        return [(77, 31, 32)]
    return positions(n, H, W, c["rows"], c["cols"])


def case_poison(name, pos):
    """bool poison mask of one run, on the grid the poison goes in at (FFDNet's head: full resolution, the position's pixel (2r+1, 2c))."""
    c = CASES[name]
    n, H, W = c["shape"]
    i, r, col = pos
    f = 2 if c["src"] == "full" else 1
    p = torch.zeros(n, f * H, f * W, dtype=torch.bool)
    p[i, (f * r + 1) if f == 2 else r, f * col] = True
    return p


def case_reach(name, poison):
    """reach of one run on the OUTPUT's grid."""
    c = CASES[name]
    n, H, W = c["shape"]
    if c["src"] == "full":
        return reach_head(poison, H, W, c["tile"])
    if c["dst"] == "full":
        return reach_tail(poison, H, W, c["tile"])
    return reach(poison, H, W, c["tile"])
