"""The case table of the STN kernel tests (tests/test_stn_ref.py on the CPU,
tests/test_gpu_stn.py on the device): shapes chosen by reading the run-time
dispatch of csrc/stn.hip (stn_bwd_kernel / stn_bwd_image), the theta kinds,
and ``dispatch``, the restatement of that dispatch the CPU test uses to prove
that each case reaches the path it is listed for."""
import zlib
from dataclasses import dataclass

import numpy as np

F = np.float32

KINDS = ("aligned", "flipped", "sheared", "outside", "large", "tiny")


@dataclass(frozen=True)
class Case:
    hin: int
    win: int
    hout: int
    wout: int
    path: str                 # dispatch of an aligned theta with dU, see dispatch()
    why: str
    n: int = 5                # images of the aligned kind (sheared takes 14 - n)
    scale: tuple = (0.5, 0.95)  # aligned scales
    kinds: tuple = KINDS

    @property
    def name(self):
        return f"{self.hin}x{self.win}-{self.hout}x{self.wout}"


CASES = (
    Case(28, 28, 50, 50, "regs+sdu", "the model's write backward", n=9,
         kinds=KINDS + ("zoom",)),
    Case(20, 12, 64, 40, "regs+sdu", "non-square, Win <= 32, Hout = 64"),
    Case(24, 40, 30, 64, "regs+sdu", "Win > 32 and Hin > 16: du_mode without upre", n=9),
    Case(8, 8, 64, 64, "regs+sdu", "more than 8 canvas columns per source column",
         scale=(0.6, 0.9), kinds=("aligned", "sheared", "tiny")),
    Case(40, 28, 50, 64, "sdu", "Hin*Win > 1024: no regs; Hin > 32: du_mode without upre"),
    Case(50, 50, 28, 28, "sdu", "two rows per pass", n=9),
    Case(7, 9, 20, 24, "sdu", "scalar staging (Hin*Win % 4 != 0), two rows per pass"),
    Case(5, 5, 9, 11, "sdu", "scalar staging, odd Hout with two rows per pass", n=9),
    Case(40, 40, 50, 50, "atomic-aligned", "Hout > 32 with Win > 32"),
    Case(70, 20, 30, 30, "atomic-aligned", "Hin > 64"),
    Case(28, 28, 40, 70, "atomic-aligned", "Wout > 64: the column loop", n=9),
    Case(12, 20, 70, 33, "atomic-general", "Hout > 64 turns sep off for aligned theta"),
    Case(1, 1, 4, 4, "sdu", "Hin == Win == 1"),
    Case(1, 6, 5, 5, "sdu", "Hin == 1"),
    Case(6, 1, 5, 5, "sdu", "Win == 1"),
    Case(7, 5, 1, 6, "sdu", "Hout == 1"),
    Case(9, 12, 6, 1, "sdu", "Wout == 1"),
    Case(72, 72, 20, 20, "atomic-aligned", "with dU one wave per workgroup (wpb = 1)"),
    Case(60, 60, 20, 20, "sdu", "with dU two waves per workgroup (wpb = 2)"),
)
# in a test of its own: the LDS slice with dU is above 64 KiB
BIG = Case(100, 100, 16, 16, "atomic-aligned", "LDS slice above 64 KiB", n=5)

CASE_KINDS = [(c, k) for c in CASES for k in c.kinds]
CASE_KIND_IDS = [f"{c.name}-{k}" for c, k in CASE_KINDS]

# aligned images 1..4 are centred on an edge of the source: clipped on that side
SIDES = ("left", "right", "top", "bottom")
OUTSIDE_T = ((4, 0), (-4, 0), (0, 4), (0, -4), (4, -4))


def n_images(case, kind):
    return {"aligned": case.n, "flipped": 5, "sheared": 14 - case.n, "outside": 5, "large": 1,
            "tiny": 1, "zoom": 5}[kind]


def _rng(case, kind, salt=0):
    return np.random.default_rng(zlib.crc32(f"{case.name}/{kind}/{salt}".encode()))


def thetas(case, kind):
    """[N, 6] fp32, every image a different theta of the kind."""
    N = n_images(case, kind)
    rng = _rng(case, kind)
    z = np.zeros(N)
    sgn = lambda: rng.choice([-1.0, 1.0], N)  # noqa: E731
    if kind in ("aligned", "zoom"):
        lo, hi = case.scale if kind == "aligned" else (0.3, 0.42)
        sx, sy = rng.uniform(lo, hi, N), rng.uniform(lo, hi, N)
        tx, ty = rng.uniform(-0.6, 0.6, N), rng.uniform(-0.6, 0.6, N)
        tx[0], ty[0] = (1 - sx[0]) * 0.3, -(1 - sy[0]) * 0.5   # wholly inside
        if kind == "aligned":
            for i, (ex, ey) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1)), 1):
                if i < N:
                    tx[i] = ex * rng.uniform(0.95, 1.05) if ex else tx[i] * 0.3
                    ty[i] = ey * rng.uniform(0.95, 1.05) if ey else ty[i] * 0.3
        th = [sx, z, tx, z, sy, ty]
    elif kind == "flipped":
        sx, sy = rng.uniform(0.5, 0.95, N), rng.uniform(0.5, 0.95, N)
        fx = np.where(np.arange(N) % 3 == 1, 1.0, -1.0)   # (-,-), (+,-), (-,+), ...
        fy = np.where(np.arange(N) % 3 == 2, 1.0, -1.0)
        th = [fx * sx, z, rng.uniform(-0.3, 0.3, N), z, fy * sy, rng.uniform(-0.3, 0.3, N)]
    elif kind == "sheared":
        th = [rng.uniform(0.5, 0.9, N), sgn() * rng.uniform(0.05, 0.3, N),
              rng.uniform(-0.4, 0.4, N), sgn() * rng.uniform(0.05, 0.3, N),
              rng.uniform(0.5, 0.9, N), rng.uniform(-0.4, 0.4, N)]
    elif kind == "outside":
        t = np.array([OUTSIDE_T[i % 5] for i in range(N)], float)
        th = [rng.uniform(0.5, 0.9, N), z, t[:, 0], z, rng.uniform(0.5, 0.9, N), t[:, 1]]
    elif kind == "large":
        th = [rng.uniform(2.5, 3.0, N), z, rng.uniform(-0.2, 0.2, N), z, rng.uniform(2.5, 3.0, N),
              rng.uniform(-0.2, 0.2, N)]
    elif kind == "tiny":
        th = [z + 0.02, z, rng.uniform(-0.5, 0.5, N), z, 0.02 * rng.uniform(0.9, 1.1, N),
              rng.uniform(-0.5, 0.5, N)]
    else:
        raise ValueError(kind)
    return np.stack(th, 1).astype(F)


def inputs(case, kind, zeros=False):
    """U in (0, 1) (it doubles as a sigmoid output), a normal cotangent G and
    a per-image gscale.  ``zeros``: a tenth of G is exactly 0, and gscale is 0
    on every third image (image 0 included)."""
    N = n_images(case, kind)
    rng = _rng(case, kind, 1)
    U = rng.uniform(0.02, 0.98, (N, case.hin, case.win)).astype(F)
    G = rng.standard_normal((N, case.hout * case.wout)).astype(F)
    gs = rng.uniform(0.25, 1.5, N).astype(F)
    if zeros:
        G[rng.random(G.shape) < 0.1] = 0.0
        gs[::3] = 0.0
    return U, thetas(case, kind), G, gs


# --------------------------------------------------------------------------
# the dispatch of stn_bwd_kernel, restated from its conditions
def lds_slice(Hin, Win, Hout, Wout, dU):
    """stn_bwd_slice: floats of one wave's LDS slice."""
    hw4 = (Hin * Win + 3) & ~3
    hw_t = (Hout * Win + 3) & ~3
    atomic_l = hw4 * (2 if dU else 1) + 4 * Hout
    sep_l = max(hw4, hw_t) + 4 * 64 + 4 * 64 + 2 * 64
    return sep_l if dU and atomic_l < sep_l else atomic_l


def dispatch(th, Hin, Win, Hout, Wout, want_dU=True, du_mode=0):
    """The path one image takes through stn_bwd_kernel / stn_bwd_image."""
    th = np.asarray(th, F)
    sep = bool(th[1] == 0 and th[3] == 0 and Hin < 32768 and Win < 32768 and Hout <= 64)
    sdu = bool(want_dU and sep and th[0] > 0 and th[4] > 0 and Hin <= 64 and Win <= 64
               and Hout <= (64 if Win <= 32 else 32) and Wout <= 64)
    mode = int(sep) | int(sdu) << 1 | int(want_dU) << 2
    HW = Hin * Win
    regs = bool(sep and 32 < Wout <= 64 and HW % 4 == 0 and HW <= 1024 and mode in (1, 3, 7))
    rpi = 1 if Win > 32 else 2
    slice_b = 4 * lds_slice(Hin, Win, Hout, Wout, want_dU)
    wpb = 4
    while wpb > 1 and slice_b * wpb > 80 * 1024:
        wpb -= 1
    if want_dU:
        du = "sdu" if sdu else "atomic-aligned" if sep else "atomic-general"
    else:
        du = "read-aligned" if sep else "read-general"
    return dict(sep=sep, sdu=sdu, regs=regs, mode=mode, wpb=wpb, slice_bytes=slice_b,
                path=("regs+" if regs else "") + du, staging16=HW % 4 == 0,
                windowed=mode == 1 and not regs and HW % 4 == 0,
                upre=bool(sdu and du_mode != 0 and rpi * 16 >= Hin),
                rows_per_pass=2 if Wout <= 32 else 1, passes=-(-Wout // (32 if Wout <= 32 else 64)))


def chain_lengths(Hout, Wout):
    """(K_dtheta, K_dot): the roundings between one addend and the stored sum,
    counted from bwd_pixels / bwd_rows_reg (see tests/test_gpu_stn.py)."""
    rp = 2 if Wout <= 32 else 1
    rows = -(-Hout // rp)
    passes = -(-Wout // (32 if Wout <= 32 else 64))
    return rows * passes + passes + 6 + 6, rows * passes + 6 + 1


def columns_per_source_column(geo, n):
    """max over source columns u of the live canvas columns whose corner pair
    touches u (the register T pass holds 8)."""
    x0, x1 = geo["x0"][n, 0], geo["x1"][n, 0]
    live = x0 != x1
    if not live.any():
        return 0
    return max(int((live & ((x0 == u) | (x1 == u))).sum()) for u in range(int(x1.max()) + 1))
