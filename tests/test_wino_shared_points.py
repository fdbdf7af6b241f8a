"""CPU check of the decoder's 2-tap Winograd classes in their shared-point form (csrc/srt_nn4.hip: wino_w1d<false>, wino_in2<false>, wino_out1d<3>).

F(2,2) taken on the evaluation points 0, +1, -1 is F(2,3) with a zero third tap and without the point that tap alone feeds:

    B2 = first three rows of B3 = [d0-d2, d1+d2, d2-d1]      G2 = [g0, (g0+g1)/2, (g0-g1)/2]      A2: y0 = m0+m1+m2, y1 = m1-m2

So along an axis the transformed input of a 2-tap class is a prefix of the 3-tap class's over the same 4-pixel patch, and srt_dec_wino - whose waves own both x classes
of an output-row parity - computes the 4-point rows only and issues the MFMAs of class (py, 0) on the registers of class (py, 1).
Pure numpy, float64, the sizes of tests/test_wino_algebra.py."""
import numpy as np

B3 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float)
G3 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], float)
A3 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float)
B2 = B3[:3].copy()                                                                      # [d0-d2, d1+d2, d2-d1], d3 unused
G2 = np.array([[1, 0], [.5, .5], [.5, -.5]], float)                                     # taps (g[-1], g[0])
A2 = np.array([[1, 1, 1], [0, 1, -1]], float)
BT, GT, AT = {1: B3, 0: B2}, {1: G3, 0: G2}, {1: A3, 0: A2}
SIZES = ((3, 2, 6, 8), (1, 1, 2, 4), (2, 3, 4, 4))                                       # (cin, cout, H, W) as in test_wino_algebra.py


def taps(p):                        # (input shift d, kernel index k = p + 1 - 2 d)
    return [(-1, 4), (0, 2), (1, 0)] if p == 1 else [(-1, 3), (0, 1)]


def direct(x, w):
    cout, H, W = w.shape[1], x.shape[1], x.shape[2]
    y = np.zeros((cout, 2 * H, 2 * W))
    for h in range(H):
        for ww in range(W):
            for ky in range(5):
                for kx in range(5):
                    Y, X = 2 * h + ky - 1, 2 * ww + kx - 1
                    if 0 <= Y < 2 * H and 0 <= X < 2 * W:
                        y[:, Y, X] += w[:, :, ky, kx].T @ x[:, h, ww]
    return y


def weights(w, py, px):             # U[ci][co][i][j] of class (py, px)
    g = np.stack([np.stack([w[:, :, ky, kx] for (_, kx) in taps(px)], -1) for (_, ky) in taps(py)], -2)
    return np.einsum('ik,cokl,jl->coij', GT[py], g, GT[px])


def points(patch, py, px):          # V[ci][i][j] of class (py, px) from the block's 4 x 4 patch (rows a0-1..a0+2, columns b0-1..b0+2)
    return np.einsum('ik,ckl,jl->cij', BT[py], patch, BT[px])


def winograd(x, w):
    cin, cout, H, W = x.shape[0], w.shape[1], x.shape[1], x.shape[2]
    xp = np.zeros((cin, H + 3, W + 3))
    xp[:, 1:H + 1, 1:W + 1] = x
    y = np.zeros((cout, 2 * H, 2 * W))
    npts = 0
    for py in (1, 0):
        for px in (1, 0):
            U = weights(w, py, px)
            npts += U.shape[2] * U.shape[3]
            for a0 in range(0, H, 2):
                for b0 in range(0, W, 2):
                    V = points(xp[:, a0:a0 + 4, b0:b0 + 4], py, px)
                    Yb = np.einsum('ik,okl,jl->oij', AT[py], np.einsum('coij,cij->oij', U, V), AT[px])
                    for da in range(2):
                        for db in range(2):
                            y[:, 2 * (a0 + da) + py, 2 * (b0 + db) + px] = Yb[:, da, db]
    return y, npts


def test_shared_point_matrices_reproduce_the_transposed_convolution():
    rng = np.random.default_rng(7)
    for (cin, cout, H, W) in SIZES:
        x = rng.standard_normal((cin, H, W))
        w = rng.standard_normal((cin, cout, 5, 5))
        y, npts = winograd(x, w)
        assert npts == 49                                   # the U layout keeps its 16 + 12 + 12 + 9 points
        assert np.abs(y - direct(x, w)).max() < 1e-12


def test_two_tap_form_is_three_tap_form_with_a_zero_tap():
    g = np.array([0.7, -1.3])
    assert np.array_equal((G3 @ np.array([g[0], g[1], 0.0]))[:3], G2 @ g) and (G3 @ np.array([g[0], g[1], 0.0]))[3] == 0.0
    assert np.array_equal(B2, B3[:3]) and np.array_equal(A2[0], A3[0, :3]) and np.array_equal(A2[1], A3[1, :3])


def test_every_point_of_class_py0_is_a_point_of_class_py1():
    """value (i, j) of class (py, 0) is value (i, j) of class (py, 1) of the same block, bit for bit: the kernel keeps one register for both"""
    rng = np.random.default_rng(13)
    for (cin, _, H, W) in SIZES:
        x = rng.standard_normal((cin, H, W))
        xp = np.zeros((cin, H + 3, W + 3))
        xp[:, 1:H + 1, 1:W + 1] = x
        for a0 in range(0, H, 2):
            for b0 in range(0, W, 2):
                patch = xp[:, a0:a0 + 4, b0:b0 + 4]
                for py in (1, 0):
                    v1, v0 = points(patch, py, 1), points(patch, py, 0)
                    assert v1.shape[1:] == ((4, 4) if py else (3, 4)) and v0.shape[1:] == ((4, 3) if py else (3, 3))
                    assert np.array_equal(v0, v1[:, :, :3])
                # (and along y: the even output rows' values are the first three rows of the odd rows' - srt_dec_wino32's class waves do not use it)
                assert np.array_equal(points(patch, 0, 1), points(patch, 1, 1)[:, :3, :])
