"""numpy restatement of the three-piece bf16 GEMM of csrc/gemm_split.hip (gemm_split3i_kernel) and of its operand layout (csrc/split3_layout.h).

An f32 value splits into three bf16 pieces by repeated round-to-nearest-even; every residual is exact in f32.  A product of two pieces (8 x 8 significand
bits) is exact, so a 16-k block of one product is summed here in float64 and then added to the f32 accumulator: one f32 rounding per product and 16-k block,
which is what the MFMA's f32 accumulator does.  Product order inside a block = the kernel's: smallest first.
"""
import numpy as np

# (plane of A, plane of B), in the kernel's accumulation order
PRODUCTS = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]
TWO_PIECE = [(0, 1), (1, 0), (0, 0)]


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def pieces(x, n=3):
    """n bf16 pieces of x (float32 arrays) and the float32 residual left behind them"""
    r = np.asarray(x, np.float32).copy()
    out = []
    for _ in range(n):
        p = bf16_rne(r)
        out.append(p)
        r = (r - p).astype(np.float32)
    return out, r


def gemm(A, B, products=PRODUCTS, npieces=3):
    """C[M][N] = A[M][K] . B[N][K]^T on `npieces` bf16 pieces per operand, the listed piece products, f32 accumulation per product and 16-k block"""
    a, _ = pieces(A, npieces)
    b, _ = pieces(B, npieces)
    a = [p.astype(np.float64) for p in a]
    b = [p.astype(np.float64) for p in b]
    M, K = A.shape
    acc = np.zeros((M, B.shape[0]), np.float32)
    for k0 in range(0, K, 16):
        for pa, pb in products:
            blk = a[pa][:, k0:k0 + 16] @ b[pb][:, k0:k0 + 16].T      # exact products, float64 sum of 16
            acc = (acc.astype(np.float64) + blk).astype(np.float32)
    return acc


def inputs(M, N, K, ncomp=1, seed=0):
    """A ~ N(0, 1), B ~ U(+-1 / sqrt(K)), float32, seeded by the shape"""
    rs = np.random.RandomState(seed + 1000003 * M + 10007 * N + 101 * K + ncomp)
    A = rs.standard_normal((ncomp, M, K)).astype(np.float32)
    B = (rs.uniform(-1.0, 1.0, (ncomp, N, K)) / np.sqrt(K)).astype(np.float32)
    return A, B


def err(C, ref64):
    """max-abs error against the float64 product, over max |float64 product|"""
    return float(np.abs(np.asarray(C, np.float64) - ref64).max() / np.abs(ref64).max())


def bar(A, B, ref64):
    """3 x the error of numpy's float32 product on the same inputs"""
    native = np.matmul(A, np.swapaxes(B, -1, -2))
    assert native.dtype == np.float32
    return 3.0 * err(native, ref64)


# ---- operand layout (csrc/split3_layout.h): [row / 2][k / 32][row % 2][plane][k % 32] ----
def rows_padded(rows):
    return (rows + 1) & ~1


def comp_elems(rows, K):
    return rows_padded(rows) * K * 3


def index(row, k, plane, K):
    return ((row >> 1) * (K // 32) + (k >> 5)) * 192 + (row & 1) * 96 + plane * 32 + (k & 31)


def to_layout(X):
    """f32 [rows][K] -> the uint16 image the writers produce (pad row of an odd matrix left at 0xFFFF)"""
    rows, K = X.shape
    p, res = pieces(X)
    assert not res.any()
    out = np.full(comp_elems(rows, K), 0xFFFF, np.uint16)
    r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    for pl in range(3):
        out[index(r, k, pl, K)] = (p[pl].view(np.uint32) >> 16).astype(np.uint16)
    return out


def from_layout(img, rows, K):
    r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    X = np.zeros((rows, K), np.float32)
    for pl in reversed(range(3)):   # smallest piece first: the sum is exact in this order for values that split exactly
        X = X + (img[index(r, k, pl, K)].astype(np.uint32) << 16).view(np.float32)
    return X
