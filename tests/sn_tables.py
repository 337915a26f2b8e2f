"""TEST INFRASTRUCTURE ONLY -- mg_sn_power_iteration driven directly from a hand-built mg_sn_layer table.

``run(layers, do_power_iteration, eps, device)`` takes a list of ``Layer`` (W [rows, cols], u [rows], v [cols] as CPU fp32 tensors, plus
the flags "give u_copy / v_copy" and "start W four bytes past a 16-byte boundary"), allocates what the header asks for per layer
(t1 [cols], t2 [rows], partial [mg_sn_layer_blocks(rows, cols, 2)][cols], sigma [1], the two copies) with a guard region on either side of
every buffer (tests/guard_alloc.py), fills scratch and outputs with an all-ones NaN, builds the table with ops.DeviceTable and the two block
maps with ops.block_map from mg_sn_layer_blocks(.., 0 / 1) of the backend IN USE (first_block_k1 / _k3 = running sums), calls the entry
point once and returns every buffer on the CPU together with the guard verdict.  No nn.Module, no SpectralPlan.

The reference side is here as well: ``contract`` (the formulas of oracle/cabi_emulator.py::mg_sn_power_iteration in float64, with t1 and
t2 returned), the seeded operand generators of the test groups, and the precondition figures under which a group's operands make every
fp32 sum exact in any order (integers below 2^24).  tests/test_sn_tables.py checks those preconditions without any backend.
"""
from __future__ import annotations

import numpy as np
import torch

import guard_alloc as GA

EXACT = 1 << 24                       # every integer of magnitude <= 2^24 is an fp32 value; sums that stay below are exact in any order
NAN_BITS = -1                         # int32 view of the sentinel: 0xFFFFFFFF, a NaN (what guard_alloc fills with)
EPS_EXACT = 4096.0                    # group B: 2^12 = sqrt(2^24), above every norm that passes chain_figures' bounds

# (rows, cols, W starts 4 bytes past a 16-byte boundary) -- the smallest shapes that cross each boundary of the four kernels
# (K1: 128 rows x 1024 columns per workgroup; K2 / K4: 1024-thread strides; K3: 4 rows per workgroup, 256 columns per trip)
BOTH_LARGE = (1029, 2052, False)
LAYER_SET = [
    (130, 2052, False),               # chunks 128 + 2; 3 column blocks, the last 4 columns wide; 3 trips of K2; 9 trips of K3, the last ragged
    (129, 27, False),                 # 4-byte fallback (cols & 3) with two chunks
    BOTH_LARGE,                       # 9 chunks x 3 column blocks at once (8 MB)
    (5, 27, False),                   # fewer rows than two K3 workgroups hold; fallback
    (1, 8, False),                    # a single row
    (257, 1026, False),               # cols & 3 != 0 with two column blocks and three chunks: the c + j < cols guards
    (128, 1024, False),               # exactly one chunk, one column block, nothing ragged
    (130, 1028, True),                # cols & 3 == 0 but W is misaligned: fallback by the pointer test, in K1 and in K3
    (1029, 36, False),                # > 1024 rows: second trip of K4; 8 full chunks + 5 rows; 257 K3 workgroups + 1 row
]
NO_COPIES = (257, 1026)               # the layer of every group that runs with u_copy = v_copy = null


class Layer:
    def __init__(self, w, u, v, copies=True, misalign=False):
        self.w, self.u, self.v = w.contiguous().float(), u.contiguous().float(), v.contiguous().float()
        self.rows, self.cols = self.w.shape
        assert self.u.shape == (self.rows,) and self.v.shape == (self.cols,)
        self.copies, self.misalign = copies, misalign

    def __repr__(self):
        return "%dx%d%s%s" % (self.rows, self.cols, "+4B" if self.misalign else "", "" if self.copies else " no copies")


# ---- operands --------------------------------------------------------------------------------------------------------------------------
def _gen(rows, cols, tag):
    return torch.Generator().manual_seed(1000003 * tag + 4099 * rows + cols)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse_ints(shape, density, g):
    """Integers of -2, -1, 1, 2 at `density`, zero elsewhere."""
    mag = torch.randint(1, 3, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    return mag * (torch.rand(shape, generator=g) < density).float() + 0.0       # + 0.0: no -0 among the zeros


def _layer(w, u, v, rows, cols, misalign):
    if rows == 1 and float(u[0]) == 0:
        u = torch.ones(1)                # a single row with u = 0 would test nothing
    return Layer(w, u, v, copies=(rows, cols) != NO_COPIES, misalign=misalign)


def eval_exact_layer(rows, cols, misalign=False):
    """Group A: dense W in -2..2, u and v in {-1, 0, 1}."""
    g = _gen(rows, cols, 1)
    return _layer(_ints((rows, cols), -2, 2, g), _ints((rows,), -1, 1, g), _ints((cols,), -1, 1, g), rows, cols, misalign)


def chain_exact_layer(rows, cols, misalign=False, density=0.08):
    """Group B: W in -2..2 at `density`, u in {-1, 0, 1} with half of it zero; v (overwritten) in {-1, 0, 1}.
    (W t1)[r] carries the term u[r] * sum_c W[r][c]^2, about 2.5 * density * cols: its square over the rows with u != 0 is what takes
    sum (W t1)^2 towards 2^24 for the wide layers, hence the sparse W and the half-empty u."""
    g = _gen(rows, cols, 2)
    w = _sparse_ints((rows, cols), density if rows * cols >= 4096 else 0.5, g)      # a small layer at 8 % would be all but empty
    u = (torch.randint(0, 2, (rows,), generator=g) * 2 - 1).float() * torch.randint(0, 2, (rows,), generator=g).float()
    return _layer(w, u, _ints((cols,), -1, 1, g), rows, cols, misalign)


def dense_int_layer(rows, cols, misalign=False):
    """Group C: dense W in -2..2, u in {-1, 0, 1}; v (overwritten) seeded normals."""
    g = _gen(rows, cols, 3)
    return _layer(_ints((rows, cols), -2, 2, g), _ints((rows,), -1, 1, g), torch.randn(cols, generator=g), rows, cols, misalign)


def realistic_layer(rows, cols, misalign=False):
    """Group D: W seeded normals x 0.05, u and v normalised normal vectors."""
    g = _gen(rows, cols, 4)
    w = torch.randn(rows, cols, generator=g) * 0.05
    u, v = torch.randn(rows, generator=g), torch.randn(cols, generator=g)
    return _layer(w, u / u.norm(), v / v.norm(), rows, cols, misalign)


def layer_set(make, skip=()):
    return [make(r, c, mis) for (r, c, mis) in LAYER_SET if (r, c, mis) not in skip]


# ---- preconditions of the exact groups (integer arithmetic, no backend) --------------------------------------------------------------------
def _i64(t):
    i = t.to(torch.int64)
    assert torch.equal(i.to(t.dtype), t), "operand is not integer valued"
    return i


def eval_figures(layer):
    """Group A: max_r sum_c |W v| and sum_r |u (W v)|; both below 2^24 make t2 and sigma exact in any summation order."""
    w, u, v = _i64(layer.w), _i64(layer.u), _i64(layer.v)
    t2 = w @ v
    return {"max_r sum_c |W v|": int((w.abs() @ v.abs()).max()), "sum_r |u t2|": int((u * t2).abs().sum())}


def chain_figures(layer):
    """Groups B and C, in units of the integers involved (B divides by powers of two only, which changes no significand):
    t1 = W^T u, ss1 = sum t1^2, W t1, ss2 = sum (W t1)^2; ss2 also bounds every partial sum of sigma = u . t2 and every product in it."""
    w, u = _i64(layer.w), _i64(layer.u)
    t1 = w.t() @ u
    wt1 = w @ t1
    return {"max_c sum_r |W u|": int((w.abs().t() @ u.abs()).max()), "sum t1^2": int((t1 * t1).sum()),
            "max_r sum_c |W t1|": int((w.abs() @ t1.abs()).max()), "sum (W t1)^2": int((wt1 * wt1).sum())}


def exact(figures, keys=None):
    return all(v < EXACT for k, v in figures.items() if keys is None or k in keys)


T1_KEYS = ("max_c sum_r |W u|", "sum t1^2")             # what group C needs: t1, partial and ss1 exact


# ---- the contract in float64 ---------------------------------------------------------------------------------------------------------------
def contract(w, u, v, do_power_iteration, eps):
    """torch/nn/utils/spectral_norm.py compute_weight (dim 0, one iteration) on fp32 operands in float64 arithmetic, as the emulator
    states it: v and u are stored as fp32 (one rounding) and read back for t2 and sigma.  A dict: t1, t2, sigma [1] float64, u and v
    fp32 (t1 is None in eval mode, where u and v are the inputs)."""
    w, u, v = w.double(), u.float(), v.float()
    t1 = None
    if do_power_iteration:
        t1 = w.t() @ u.double()
        v = (t1 / max(float(t1.norm()), eps)).float()
        t2 = w @ v.double()
        u = (t2 / max(float(t2.norm()), eps)).float()
    else:
        t2 = w @ v.double()
    return {"t1": t1, "v": v, "t2": t2, "u": u, "sigma": (u.double() @ t2).reshape(1)}


def held_by_fp32(t):
    """Every value of the float64 tensor is an fp32 value: the cast loses nothing."""
    return torch.equal(t.float().double(), t)


# ---- a-priori bounds for realistic operands (derivation: module docstring of tests/test_gpu_sn_power_iteration.py) --------------------------
U = 2.0 ** -24                        # unit roundoff of fp32
K1_ROWS = 128                         # rows per W^T u partial (michigan_amd/csrc/mg_weights.hip)


def _ceil(a, b):
    return -(-a // b)


def adds_t1(rows):
    return min(rows, K1_ROWS) + _ceil(rows, K1_ROWS)             # a thread's sequential sum over its chunk's rows, then one add per chunk


def adds_t2(cols):
    return _ceil(cols, 256) + 2 + 6                               # trips of the 256-column stride, (a0 + a1) + (a2 + a3), the wave tree


def adds_block(n):
    return _ceil(n, 1024) + 6 + 15                                # a thread's trips, the wave tree, the 16 wave sums joined left to right


def bound_t1(w, u):
    """Per column: |t1 - W^T u| <= (d + 1) U sum_r |W[r][c] u[r]|."""
    return (adds_t1(w.shape[0]) + 1) * U * (w.double().abs().t() @ u.double().abs())


def bound_t2(w, v):
    """Per row: |t2 - W v| <= (d + 1) U sum_c |W[r][c] v[c]|."""
    return (adds_t2(w.shape[1]) + 1) * U * (w.double().abs() @ v.double().abs())


def rel_bound_normalise(n):
    """Relative, per element: ss carries (d + 1) U, the square root halves that and rounds once, the quotient rounds once."""
    return ((adds_block(n) + 1) / 2 + 2) * U


def bound_sigma(u, t2):
    return (adds_block(u.numel()) + 1) * U * float((u.double() * t2.double()).abs().sum())


def normalise64(t, eps):
    t = t.double()
    return t / max(float(t.norm()), eps)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


def untouched(t):
    """The sentinel is still in every element."""
    return bool((bits(t) == NAN_BITS).all())


# ---- the device side -----------------------------------------------------------------------------------------------------------------------
def run(layers, do_power_iteration, eps, device):
    """One mg_sn_power_iteration over `layers` on the current backend.  Returns a dict:
    layers   per layer a dict of CPU tensors u, v, t1, t2, partial [chunks, cols], sigma, u_copy, v_copy (None where not given) and w
    k1, k3   workgroups per layer for the two streaming kernels; first_k1, first_k3 the running sums written to the table
    map1, map3   the block maps (CPU);  calls  the mg_* entry points called, in order;  guards  None, or the damage report"""
    from michigan_amd import _cabi as C, ops

    with GA.guard() as g:
        be = C.backend()
        n = len(layers)
        table = ops.DeviceTable(C.SnLayer, n, device)
        rows_tab = table.begin_update()
        k1, k3, first1, first3, bufs = [], [], [], [], []
        b1 = b3 = 0

        def scratch(numel):
            t = g.guarded(numel, torch.float32, device)
            bits(t).fill_(NAN_BITS)
            return t

        for L, r in zip(layers, rows_tab):
            rows, cols = L.rows, L.cols
            chunks = int(be.mg_sn_layer_blocks(rows, cols, 2))
            assert chunks > 0
            if L.misalign:
                flat = g.guarded(rows * cols + 1, torch.float32, device)
                w = flat[1:].view(rows, cols)
                assert w.data_ptr() % 16 == 4
            else:
                w = g.guarded((rows, cols), torch.float32, device)
                assert w.data_ptr() % 16 == 0
            w.copy_(L.w)
            b = {"w": w, "u": g.place(L.u, device), "v": g.place(L.v, device), "t1": scratch(cols), "t2": scratch(rows),
                 "partial": scratch(chunks * cols), "sigma": scratch(1),
                 "u_copy": scratch(rows) if L.copies else None, "v_copy": scratch(cols) if L.copies else None, "chunks": chunks}
            for name in ("w", "u", "v", "u_copy", "v_copy", "sigma", "t1", "t2", "partial"):
                setattr(r, name, b[name].data_ptr() if b[name] is not None else None)
            r.rows, r.cols, r.first_block_k1, r.first_block_k3 = rows, cols, b1, b3
            k1.append(int(be.mg_sn_layer_blocks(rows, cols, 0)))
            k3.append(int(be.mg_sn_layer_blocks(rows, cols, 1)))
            first1.append(b1)
            first3.append(b3)
            b1 += k1[-1]
            b3 += k3[-1]
            bufs.append(b)
        map1, map3 = ops.block_map(k1, device), ops.block_map(k3, device)
        status = be.mg_sn_power_iteration(table.upload(), n, ops._p(map1), b1, ops._p(map3), b3, 1 if do_power_iteration else 0, float(eps),
                                          ops._stream(map3))
        assert not status, "mg_sn_power_iteration returned %r" % (status,)
        try:
            g.check()
            verdict = None
        except GA.GuardDamaged as e:
            verdict = str(e)
        out = []
        for b in bufs:
            o = {k: (t.detach().cpu().clone() if torch.is_tensor(t) else t) for k, t in b.items()}
            o["partial"] = o["partial"].view(b["chunks"], -1)
            out.append(o)
        return {"layers": out, "k1": k1, "k3": k3, "first_k1": first1, "first_k3": first3, "map1": map1.cpu(), "map3": map3.cpu(),
                "nblocks": (b1, b3), "calls": list(g.backend.calls), "guards": verdict}


def f32_normalise(t, ss_exact, eps):
    """t / max(sqrt(ss), eps) evaluated in fp32 with numpy (correctly rounded square root and quotient); ss is given exactly."""
    assert 0 <= ss_exact < EXACT
    denom = max(np.sqrt(np.float32(ss_exact)), np.float32(eps))
    return torch.from_numpy(t.numpy().astype(np.float32) / np.float32(denom))
