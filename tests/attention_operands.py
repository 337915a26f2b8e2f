"""Operands for which mg_self_attention (csrc/mg_attention.hip) has an EXACT value, a per-element error bound where it has not, and a
CPU model of the kernel's dataflow whose one-line mutations show that the comparisons of tests/test_gpu_attention_exact.py bite.

Exact operands.  exp2((s - m) * log2e) is exactly 0 once m - s >= 128 (128 * log2(e) = 184.7 > 150: below half the smallest fp32 denormal,
and zero under flush-to-zero as well) and exactly 1 at s = m.  Scores whose top value is 128 or more above every key outside a selected set,
and equal inside it, turn the softmax into weights in {0, 1}: the kernel is then a gather (one selected key) or a class mean (a power-of-two
number of them, integer values, sums below 2^24) and has to return the stored bits / the once-rounded float64 mean, whatever the rounding
of exp2, of the rescale or of the summation order.  Whatever the accumulators held before a query's top key arrived is multiplied by
alpha = exp2(-184.7 or less) = 0.
  codes      row j of a seeded +-1 matrix [L, 63] times 8; dimension 63 carries an offset, q[..., 63] = 64 and k[..., 63] = -128 * neg.
             Two codes that differ in one position are 2 * 64 = 128 apart.  neg = 1: every real score is at most 63 * 64 - 8192 < 0, so
             that a key past L that escapes the mask (a zero-filled K row: score 0) would win the maximum.
  gather     q_i = code(perm(i)), k_j = code(j), v arbitrary finite values with -0.0 and exact zeros: the reference is v[:, perm].
  classes    the keys are partitioned into classes whose sizes are the powers of two of L's binary expansion, members spread over the
             tiles by a seeded shuffle (keys 0 and L - 1 share the largest class); k_j = code(class(j)), query i takes class i % nclasses,
             v integers in [-255, 255] (exact in bf16; sums stay at or below 255 * 4096 < 2^24): the reference is the float64 class mean,
             rounded once.  (Integers in [-8, 8] would not do: a mean of s of them has a numerator of at most 8 s, which fits bf16's 8
             significant bits up to s = 32, so that below L = 64 no output would need rounding and a wrongly rounded mean could not show.
             With 8 bits per value a sum of two already needs rounding.)  At least 5 % of the bf16 outputs of the classes of 8 and more
             keys need rounding.
Preconditions (asserted on the float64 scores before a kernel's result is looked at): for every query the top score is 128 or more above
the best score outside its selected set, all |s| <= 2^24 (fp32 holds them exactly, in any summation order).

Weighted operands.  "realistic": the recipe of test_self_attention_matches_contract (normal q, k times `scale`, one key planted near the end
that dominates query 7).  "pairs": the keys come in pairs (a, b) that share a code, sit in different key tiles and in different half-wave
slots (wherever L has room for that), with v_a = +X, v_b = -X; dimension 62 holds k_a = +1/8, k_b = -1/8 and q_i = r_i in 1..8, so that
s_ia - s_ib = r_i / 4 and the output is X * tanh(r_i / 8): numerator terms cancel, and on more than half of the elements |out| is below a
quarter of sum_j P_ij |v_j|.  Every other key is 128 or more below the pair.

The bound.  With float64 P_ij (softmax), ref = P v, A_ic = sum_j P_ij |v_jc|, T_i = max_j sum_d |q_id k_jd|, D_i = the largest m_i - s_ij among
keys with P_ij >= 2^-40, and u = 2^-24, the kernel computes  out = fl(N / l)  with  N = sum_j p_j v_j,  l = sum_j p_j,  p_j the kernel's weights
relative to the final maximum.  One term per rounding (line numbers of csrc/mg_attention.hip):
  score        (145 / 154) 64 products accumulated in fp32.  fp32 path: the MFMA is a k-ordered fmaf chain, one rounding (u) per product.
               bf16 path: products are exact, the MFMA's internal additions are not documented: one ulp (2 u) per term.
               |ds| <= 64 c u T_i.  When q and k are multiples of powers of two with T_i below 2^24 quanta ("pairs", the exact operands) every
               partial sum is exact and the term is 0.  It moves a weight, relative to the row maximum's, by expm1(2 ds).
  argument     (188, 175) x = (s - m) * LOG2E: the subtraction, the fp32 constant (off by 1.3e-8 < u) and the product, 3 u |x|; a key meets
               one such argument when it is exponentiated and one per later rescale, whose lengths add up to m_i - s_ij: 3 u D_i on its weight.
  exp2         (188, 175) v_exp_f32, ASSUMED accurate to 2 ulp (2^-22 relative; its accuracy is not documented where this was written): once
               per key and once per rescale that follows, (1 + R_i) 2^-22 with R_i the number of key tiles that raise the running maximum to
               within 110 of the final one (earlier rescales scale what alpha = 0 wipes or what stays below e^-110 of the result).
  split        (210-211) bf16 only: p = hi + lo with lo = bf16(p - hi), |p - hi - lo| <= 2^-8 |p - hi| <= 2^-16 p.  Numerator only: l sums the fp32 p.
  accumulate   numerator (226-227 bf16: one MFMA chain, hi and lo terms; 250, 255 fp32: 32 keys from zero, then one add per tile): a term
               whose weight is exactly 0 adds exactly nothing, so what counts is n_i = the number of keys within 110 of the RUNNING maximum
               of their tile (the others are exp2(< -150) = 0 in the kernel).  bf16: 2 n_i terms at one ulp each, (2 n_i) 2 u A; fp32:
               (min(32, n_i) + min(tiles, n_i)) u A.  Row sum (188, 266): n_i + 1 fp32 additions, (n_i + 1) u l.
  rescale      (176, 180) one product per rescale on l and on every accumulator: R_i u each.
  1 / l, mult  (267, 276) a division (one ulp allowed: 2 u) and a product (u), relative to |ref|.
  negligible   keys with P < 2^-40 may be flushed, wiped or wrong by any factor below 2: 2^-39 sum_j |v_jc| in the numerator, L 2^-40 in l.
Every factor (1 + e) on a weight compounds to at most exp(w_i), w_i = 2 ds + 3 u D_i + (1 + R_i) 2^-22; weight errors act on the numerator (times
A) and on the row sum (times |ref|): they count twice.  With the computed row sum l (1 + t), |t| <= theta_i, and N + dN:
  EN_i    = expm1(w_i + split + acc_num_i + R_i u)                  |dN_ic| <= EN_i A_ic + 2^-39 sum_j |v_jc|
  theta_i = expm1(w_i + (n_i + 1 + R_i) u + 3 u) + L 2^-40          (the 3 u of 1 / l and the last product ride along; theta_i < 1/2 is asserted)
  b_ic    = (EN_i A_ic + 2^-39 sum_j |v_jc| + theta_i |ref_ic|) / (1 - theta_i)          from  N^/l^ - N/l = (dN / l - t ref) / (1 + t)
b bounds the fp32 value BEFORE the store.
  store        (277) fp32: none.  bf16: round-to-nearest is monotone, so the stored value lies in [bf16(ref - b), bf16(ref + b)] and
               bound = max(|bf16(ref - b) - ref|, |bf16(ref + b) - ref|): the rounding error of ref itself wherever ref +- b does not straddle
               a rounding boundary.  (The cruder  b + 2^-8 |ref|  cannot tell a single-bf16 P from the kernel: on "pairs" at r = 1 that mutant
               is off by 1.7 to 3.4 half-ulps of the output.)
The condition that keeps the bound honest (tests/test_attention_operands.py): on "pairs" in bf16 the model WITHOUT the lo product errs by at
least 8 bounds on at least 10 % of the elements.

The model restates the kernel's dataflow in torch fp32, vectorised over the queries: key tiles of KVB, the two LDS buffers alternating, key
slot 8 (r >> 2) + (r & 3) + 4 hi per half-wave, the mask of keys >= L, a running maximum exchanged between the halves, a wave-uniform rescale,
per-half row sums joined at the end, the hi + lo split, the store guarded by qrow < L.  It does not reproduce the MFMA's summation order: on the
exact operands no order matters, on the weighted ones the bound covers any.  MUTANTS are one-line changes of it: ten
listed when these tests were asked for, of which "store-row-clamped" is an equivalent mutant (rows >= L recompute row L - 1 from the clamped load and
store the same bits), and "store-unguarded", which stands in for it.
"""
import functools
import math

import torch

from exact_operands import DT, LIMIT, _gen, check_distinct, ints, rounding_share

DQK, DV, BQ = 64, 256, 128
KVB = {"bf16": 64, "f32": 32}
GAP = 128.0
LOG2E = 1.4426950408889634
NEG_BIG = -1.0e30
U = 2.0 ** -24
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257, 333)
PERMS = ("identity", "reversal", "shift", "stride37", "all-to-last", "all-to-first", "shuffle")
SHUFFLE_SEED = 1000               # of the seeded shuffles: one with which the permutations of all lengths, taken together, bring every query lane
#                                    together with every key slot (tests/test_attention_operands.py asserts it; a property of the operands alone)
ROUNDING_MIN_CLASS = 8
V_CLASS_MAX = 255                  # 8 significant bits: exact in bf16, and 255 * 4096 < 2^24
REALISTIC = ((129, 0.1), (129, 3.0), (200, 1.0), (4096, 0.35))
PAIRS_L = (64, 130, 258, 4096)
# r of the "pairs" queries, dealt in this proportion: every value of 1..8, and r = 1 (p_b = e^-1/4, where the partner's weight is largest and the
# output smallest: a lost low-order part of P shows most) on 5 of 8 queries, so that |out| <= A / 4 (r <= 2) holds on more than half of them
R_DRAW = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 1, 1, 1, 1, 1, 2, 2)
MUTANTS = ("mask-gt", "mask-no-hi", "no-acc-rescale", "m-not-exchanged", "l-upper-dropped", "p-slots-swapped", "v-swizzle-and3", "lo-dropped", "stale-v-buffer",
           "store-row-clamped", "store-unguarded")
BF16_ONLY = ("v-swizzle-and3", "lo-dropped")


def half_of(key):
    """The half-wave whose accumulators hold key slot `key` of a 32-key tile: slot 8 (r >> 2) + (r & 3) + 4 hi."""
    return (key >> 2) & 1


# ---------------------------------------------------------------------------------------------------------------------
# exact operands
# ---------------------------------------------------------------------------------------------------------------------
def codes(n, width=63, seed=0):
    return (ints(_gen(4000 + 7 * n + seed), (n, width), 0, 1) * 2 - 1) * 8


def perm_index(name, L):
    i = torch.arange(L)
    if name == "identity":
        return i
    if name == "reversal":
        return L - 1 - i
    if name == "shift":
        return torch.remainder(i + L - 5, L)
    if name == "stride37" and math.gcd(37, L) == 1:
        return (37 * i) % L
    if name == "all-to-last":
        return torch.full((L,), L - 1)
    if name == "all-to-first":
        return torch.zeros(L, dtype=torch.long)
    assert name in ("shuffle", "stride37"), name
    return torch.randperm(L, generator=_gen(SHUFFLE_SEED + L + (37 if name == "stride37" else 0)))


def _with_offset(c, last):
    return torch.cat([c, torch.full((c.shape[0], 1), float(last))], 1)


def arbitrary_values(dt, N, L, seed):
    """randn (clamped to +-4) * 2^randint(-20, 20), rounded to dt, with -0.0 at 2 % and exact zeros at 2 % of the elements."""
    g = _gen(seed)
    v = torch.randn((N, L, DV), generator=g).clamp(-4, 4) * 2.0 ** ints(g, (N, L, DV), -20, 20)
    pick = torch.rand((N, L, DV), generator=g)
    v = torch.where(pick < 0.02, torch.full_like(v, -0.0), v)
    v = torch.where(pick > 0.98, torch.zeros_like(v), v)
    return v.to(DT[dt])


def check_selected(name, q, k, selected):
    """Preconditions of the exact operands on the float64 scores of one sample: selected [L, L] bool marks each query's chosen keys."""
    s = q.double() @ k.double().t()
    assert float(s.abs().max()) <= LIMIT, f"{name}: a score exceeds 2^24"
    top = s.max(1).values
    inside = torch.where(selected, s, torch.full_like(s, float("inf"))).min(1).values
    assert torch.equal(inside, top), f"{name}: the selected keys do not all hold the row maximum"
    if not bool(selected.all()):
        outside = torch.where(selected, torch.full_like(s, float("-inf")), s).max(1).values
        gap = float((top - outside).min())
        assert gap >= GAP, f"{name}: a key outside the selected set is only {gap} below the top score"
    return s


def softmax_reference(q, k, v):
    """float64 softmax(q k^T) v of [N, L, *] operands: the contract of the entry point."""
    return torch.softmax(q.double() @ k.double().transpose(1, 2), dim=-1) @ v.double()


@functools.lru_cache(maxsize=32)                                   # (read only; the float64 contract at L = 4096 costs seconds)
def gather_operands(dt, N, L, perm, neg):
    """dict(q, k, v, ref, perm): ref = v[:, perm] (no arithmetic).  The codes are shared by the samples, v differs."""
    name = f"gather {dt} N={N} L={L} {perm} neg={neg}"
    c, idx = codes(L), perm_index(perm, L)
    q = _with_offset(c[idx], 64).to(DT[dt]).expand(N, L, DQK).contiguous()
    k = _with_offset(c, -128 * neg).to(DT[dt]).expand(N, L, DQK).contiguous()
    v = arbitrary_values(dt, N, L, 11 * L + N + neg)
    assert torch.equal(q[0].double()[:, :63], c[idx].double()) and bool(torch.isfinite(v.float()).all())
    selected = torch.zeros(L, L, dtype=torch.bool)
    selected[torch.arange(L), idx] = True
    s = check_selected(name, q[0], k[0], selected)
    if neg:
        assert float(s.max()) < 0, f"{name}: a real score is not below a phantom key's 0"
    ref = v[:, idx]
    assert torch.equal(softmax_reference(q, k, v).to(DT[dt]), ref), f"{name}: the float64 contract, rounded, is not the gather"
    return dict(q=q, k=k, v=v, ref=ref, perm=idx)


def class_sizes(L):
    return [1 << b for b in range(L.bit_length() - 1, -1, -1) if L >> b & 1]


def class_of_keys(L):
    """class index per key: keys 0 and L - 1 in the largest class, the others dealt by a seeded shuffle."""
    rest = [j for j in torch.randperm(L, generator=_gen(900 + L)).tolist() if j not in (0, L - 1)]
    order = ([0] if L == 1 else [0, L - 1]) + rest
    cls = torch.empty(L, dtype=torch.long)
    at = 0
    for c, size in enumerate(class_sizes(L)):
        cls[order[at:at + size]] = c
        at += size
    assert at == L
    return cls


def class_values(dt, N, L):
    """Integers in [-255, 255]."""
    v = ints(_gen(77 + L + N), (N, L, DV), -V_CLASS_MAX, V_CLASS_MAX).to(DT[dt])
    assert torch.equal(v.double(), v.double().round()) and float(v.float().abs().max()) <= V_CLASS_MAX
    return v


def class_operands(dt, N, L, neg, kw=None):
    """dict(q, k, v, ref (float64, exact), cls, qcls).  kw [L] (test hook): a weight per key, the value a miscounting kernel would return."""
    name = f"classes {dt} N={N} L={L} neg={neg}"
    sizes, cls = class_sizes(L), class_of_keys(L)
    nc = len(sizes)
    c = codes(nc, seed=1)
    qcls = torch.arange(L) % nc
    q = _with_offset(c[qcls], 64).to(DT[dt]).expand(N, L, DQK).contiguous()
    k = _with_offset(c[cls], -128 * neg).to(DT[dt]).expand(N, L, DQK).contiguous()
    v = class_values(dt, N, L)
    assert cls[0] == cls[L - 1] == 0 and torch.equal(torch.bincount(cls, minlength=nc), torch.tensor(sizes))
    check_selected(name, q[0], k[0], cls.view(1, L) == qcls.view(L, 1))
    member = (cls.view(1, L) == torch.arange(nc).view(nc, 1)).double()            # [nc, L]
    w = member if kw is None else member * kw.double().view(1, L)
    means = (w @ v.double()) / w.sum(1).view(1, nc, 1)                            # [N, nc, DV]
    ref = means[:, qcls]
    if kw is None:
        assert float((member @ v.double().abs()).max()) < LIMIT
        if L >= 64:
            check_distinct(name, ref)
        big = torch.tensor(sizes)[qcls] >= ROUNDING_MIN_CLASS
        if dt == "bf16" and bool(big.any()):
            share = rounding_share(ref[:, big])
            assert share >= 0.05, f"{name}: only {share:.1%} of the means over {ROUNDING_MIN_CLASS} and more keys need rounding in bf16"
    return dict(q=q, k=k, v=v, ref=ref, cls=cls, qcls=qcls)


# ---------------------------------------------------------------------------------------------------------------------
# weighted operands
# ---------------------------------------------------------------------------------------------------------------------
def realistic_operands(dt, N, L, scale, seed=21):
    g = _gen(seed + L)
    q = (torch.randn(N, L, DQK, generator=g) * scale).to(DT[dt])
    k = (torch.randn(N, L, DQK, generator=g) * scale).to(DT[dt])
    v = torch.randn(N, L, DV, generator=g).to(DT[dt])
    if L > 7:
        k[:, L - 5] = (4.0 * q[:, 7].float()).to(DT[dt])               # query 7's maximum arrives in the last key tile
    return dict(q=q, k=k, v=v)


def pair_keys(L):
    """[L / 2, 2] key indices: partner a from the lower half-wave slots, b from the upper ones half the list further (another key tile)."""
    assert L % 2 == 0
    lo = [j for j in range(L) if half_of(j) == 0]
    up = [j for j in range(L) if half_of(j) == 1]
    n = min(len(lo), len(up))
    pairs = [(lo[i], up[(i + n // 2) % n]) for i in range(n)]
    left = lo[n:] + up[n:]
    pairs += [(left[i], left[i + 1]) for i in range(0, len(left), 2)]
    return torch.tensor(pairs)


def pairs_operands(dt, N, L):
    name = f"pairs {dt} N={N} L={L}"
    g = _gen(500 + L)
    pk = pair_keys(L)
    npairs = L // 2
    apart = (half_of(pk[:, 0]) != half_of(pk[:, 1])) & (pk[:, 0] // 32 != pk[:, 1] // 32)
    assert float(apart.double().mean()) >= 0.9, f"{name}: too few pairs sit in different slots and 32-key tiles"
    if L > KVB[dt]:
        assert float((pk[:, 0] // KVB[dt] != pk[:, 1] // KVB[dt]).double().mean()) >= 0.9
    c = codes(npairs, width=62, seed=2)
    qpair = torch.randperm(L, generator=g) % npairs
    r = torch.tensor(R_DRAW)[torch.randperm(L, generator=g) % len(R_DRAW)].float()
    k = torch.zeros(L, DQK)
    k[pk[:, 0], :62], k[pk[:, 1], :62] = c, c
    k[pk[:, 0], 62], k[pk[:, 1], 62] = 0.125, -0.125
    q = torch.zeros(L, DQK)
    q[:, :62], q[:, 62] = c[qpair], r
    X = torch.randn(N, npairs, DV, generator=g).to(DT[dt])
    v = torch.zeros(N, L, DV, dtype=DT[dt])
    v[:, pk[:, 0]], v[:, pk[:, 1]] = X, -X
    q, k = q.to(DT[dt]).expand(N, L, DQK).contiguous(), k.to(DT[dt]).expand(N, L, DQK).contiguous()
    s = q[0].double() @ k[0].double().t()
    rows = torch.arange(L)
    sa, sb = s[rows, pk[qpair, 0]], s[rows, pk[qpair, 1]]
    assert torch.equal(sa - sb, 0.25 * r.double()) and set(r.tolist()) == set(range(1, 9)), name
    other = s.clone()
    other[rows, pk[qpair, 0]] = float("-inf")
    other[rows, pk[qpair, 1]] = float("-inf")
    if L > 2:
        assert float((sb - other.max(1).values).min()) >= GAP, f"{name}: a key outside the pair is less than 128 below it"
    closed = X.double()[:, qpair] * torch.tanh(0.125 * r.double()).view(1, L, 1)
    return dict(q=q, k=k, v=v, closed=closed, r=r)


def weighted_operands(kind, dt, N, L, scale=1.0):
    if kind == "realistic":
        return realistic_operands(dt, N, L, scale)
    assert kind == "pairs", kind
    return pairs_operands(dt, N, L)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference with the quantities of the bound
# ---------------------------------------------------------------------------------------------------------------------
def _quantum(t):
    """The largest power of two (2^8 down to 2^-12) of which every element is a multiple; 0 when there is none."""
    t = t.double()
    for e in range(8, -13, -1):
        x = t * 2.0 ** -e
        if torch.equal(x, x.round()):
            return 2.0 ** e
    return 0.0


def _bound_one(q, k, v, dt):
    """(ref, bound) of one sample, float64 [L, DV]."""
    L, kvb, bf = q.shape[0], KVB[dt], dt == "bf16"
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.t()
    m = s.max(1, keepdim=True).values
    D = m - s
    e = torch.exp(-D)
    l = e.sum(1, keepdim=True)
    P = e / l
    ref, A = P @ v, P @ v.abs()
    T = (q.abs() @ k.abs().t()).max(1).values
    live = P >= 2.0 ** -40
    Dmax = torch.where(live, D, torch.zeros_like(D)).max(1).values
    ntiles = -(-L // kvb)
    pad = torch.full((L, ntiles * kvb - L), float("-inf"), dtype=torch.float64)
    tmax = torch.cat([s, pad], 1).view(L, ntiles, kvb).max(2).values                          # [L, ntiles]
    run = torch.cummax(tmax, 1).values
    before = torch.cat([torch.full((L, 1), float("-inf"), dtype=torch.float64), run[:, :-1]], 1)
    R = ((tmax > before) & (tmax >= m - 110)).double().sum(1) - 1                             # the first of them rescales nothing that counts
    R = R.clamp_min(0)
    run_key = run.repeat_interleave(kvb, 1)[:, :L]
    n = (s >= run_key - 110).double().sum(1)
    # score
    qq, qk = _quantum(q), _quantum(k)
    exact = qq > 0 and qk > 0 and float(T.max()) / (qq * qk) < LIMIT
    ds = torch.zeros_like(T) if exact else 64 * (2 * U if bf else U) * T
    w = 2 * ds + 3 * U * Dmax + (1 + R) * 2.0 ** -22                                          # log of the factor on a weight
    split = 2.0 ** -16 if bf else 0.0
    acc_num = (2 * n) * 2 * U if bf else (n.clamp_max(32) + n.clamp_max(ntiles)) * U
    en = torch.expm1(w + split + acc_num + R * U)
    theta = torch.expm1(w + (n + 1 + R) * U + 3 * U) + L * 2.0 ** -40
    assert float(theta.max()) < 0.5, "the row sum is not known to a factor of two: no bound"
    b = (en.view(L, 1) * A + 2.0 ** -39 * v.abs().sum(0, keepdim=True) + theta.view(L, 1) * ref.abs()) / (1 - theta).view(L, 1)
    if not bf:
        return ref, b
    lo, hi = (ref - b).float().bfloat16().double(), (ref + b).float().bfloat16().double()
    return ref, torch.maximum((lo - ref).abs(), (hi - ref).abs())


def bound(q, k, v, dt):
    """(float64 reference, per-element bound of |kernel - reference|) of [N, L, *] operands."""
    out = [_bound_one(q[i], k[i], v[i], dt) for i in range(q.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def check_pairs(name, o, ref):
    """Preconditions of the "pairs" operands on their float64 reference."""
    err = float((ref - o["closed"]).abs().max())
    assert err <= 1e-12, f"{name}: the reference is {err} away from X tanh(r / 8)"
    A = torch.softmax(o["q"].double() @ o["k"].double().transpose(1, 2), dim=-1) @ o["v"].double().abs()
    share = float((ref.abs() <= 0.25 * A).double().mean())
    assert share >= 0.5, f"{name}: only {share:.0%} of the outputs cancel to a quarter of sum P |v|"


def ratio(got, ref, bnd):
    """error / bound per element (0 / 0 = 0, x / 0 = inf)."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(err == 0, torch.zeros_like(err), err / bnd)


# ---------------------------------------------------------------------------------------------------------------------
# the CPU model of the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _model_rows(q, k, v, dt, mutate):
    """The normalised fp32 accumulators of every query row of the launch (BQ-padded: row i >= L computes with query L - 1)."""
    L, kvb, bf = q.shape[0], KVB[dt], dt == "bf16"
    Qp, ntiles = -(-L // BQ) * BQ, -(-L // kvb)
    Q = q.float()[torch.arange(Qp).clamp_max(L - 1)]
    Kp, Vp = torch.zeros(ntiles * kvb, DQK), torch.zeros(ntiles * kvb, DV)
    Kp[:L], Vp[:L] = k.float(), v.float()                              # keys past L are zero-filled in LDS
    slot = torch.arange(kvb)
    khalf, chalf = half_of(slot), half_of(torch.arange(DV))             # a 32-channel block holds channel 8 rq + 4 hi + j in half hi
    acc, m_run, l_run = torch.zeros(Qp, DV), torch.full((Qp, 2), NEG_BIG), torch.zeros(Qp, 2)
    swap = slot.clone()
    for base in range(0, kvb, 32):
        swap[base + 2], swap[base + 21] = base + 21, base + 2
    buf = [(Kp[:kvb], Vp[:kvb]), None]
    for t in range(ntiles):
        nxt = (Kp[(t + 1) * kvb:(t + 2) * kvb], Vp[(t + 1) * kvb:(t + 2) * kvb]) if t + 1 < ntiles else None
        Kt, Vt = buf[t & 1]
        if mutate == "stale-v-buffer" and t >= 2:
            Vt = buf[(t - 1) & 1][1]
        s = Q @ Kt.t()
        if t * kvb + kvb > L:
            key = t * kvb + slot - (4 * khalf if mutate == "mask-no-hi" else 0)
            s[:, (key > L) if mutate == "mask-gt" else (key >= L)] = NEG_BIG
        mloc = torch.stack([s[:, khalf == 0].max(1).values, s[:, khalf == 1].max(1).values], 1)
        if mutate != "m-not-exchanged":
            mloc = mloc.max(1, keepdim=True).values.expand(Qp, 2)
        m_new = torch.maximum(m_run, mloc)
        moved = (m_new > m_run).view(Qp // 32, 64).any(1).repeat_interleave(32).view(Qp, 1)          # wave-uniform
        alpha = torch.where(moved, torch.exp2((m_run - m_new) * LOG2E), torch.ones_like(m_run))
        l_run = l_run * alpha
        if mutate != "no-acc-rescale":
            acc = acc * alpha[:, chalf]
        m_run = torch.where(moved, m_new, m_run)
        p = torch.exp2((s - m_run[:, khalf]) * LOG2E)
        l_run = l_run + torch.stack([p[:, khalf == 0].sum(1), p[:, khalf == 1].sum(1)], 1)
        if bf and mutate == "v-swizzle-and3":                           # rows with bit 2 set read 64-byte block 5 ^ 4 for channel block 5
            Vt = Vt.clone()
            Vt[(slot & 4) != 0, 160:192] = buf[t & 1][1][(slot & 4) != 0, 32:64]
        if bf:
            ph = p.bfloat16().float()
            terms = [ph] if mutate == "lo-dropped" else [ph, (p - ph).bfloat16().float()]
        else:
            terms = [p]
        for w in terms:
            add = w @ Vt
            if mutate == "p-slots-swapped":
                add[:, 160:192] = w[:, swap] @ Vt[:, 160:192]
            acc = acc + add
        if nxt is not None:
            buf[(t + 1) & 1] = nxt
    l_tot = l_run[:, 0] if mutate == "l-upper-dropped" else l_run[:, 0] + l_run[:, 1]
    return acc * (1.0 / l_tot).view(Qp, 1)


def model(q, k, v, dt, mutate=None, tail=False):
    """out [N, L, DV] in DT[dt]; tail = True: also the BQ rows behind the last sample's (NaN where nothing was stored)."""
    assert mutate is None or mutate in MUTANTS, mutate
    N, L = q.shape[:2]
    flat = torch.full((N * L + BQ, DV), float("nan"))
    for n in range(N):
        rows = _model_rows(q[n], k[n], v[n], dt, mutate)
        flat[n * L:n * L + L] = rows[:L]
        if mutate == "store-row-clamped":                               # rows >= L recompute row L - 1 and store it there again
            for i in range(L, rows.shape[0]):
                flat[n * L + L - 1] = rows[i]
        if mutate == "store-unguarded":                                 # rows >= L land in the next sample's rows, or behind the tensor
            end = min(n * L + rows.shape[0], flat.shape[0])
            flat[n * L:end] = rows[:end - n * L]
    out = flat[:N * L].view(N, L, DV).to(DT[dt])
    return (out, flat[N * L:]) if tail else out


# ---------------------------------------------------------------------------------------------------------------------
# the comparison this suite had: test_self_attention_matches_contract's five operand sets (first sample) and tol * max|ref|
# ---------------------------------------------------------------------------------------------------------------------
OLD_SETS = ((2, 4096, 0.35), (1, 256, 1.0), (3, 200, 0.5), (1, 333, 1.5), (2, 64, 0.2))
OLD_TOL = {"f32": 2e-5, "bf16": 2.0 ** -8}


def old_operands(dt):
    """The operands of tests/test_gpu_kernels.py::test_self_attention_matches_contract, one generator through all five sets; the first sample."""
    g = torch.Generator().manual_seed(21)
    out = []
    for n, L, scale in OLD_SETS:
        q = (torch.randn(n, L, 64, generator=g) * scale).to(DT[dt])
        k = (torch.randn(n, L, 64, generator=g) * scale).to(DT[dt])
        v = torch.randn(n, L, 256, generator=g).to(DT[dt])
        k[:, L - 5] = (4.0 * q[:, 7].float()).to(DT[dt])
        out.append((q[:1], k[:1], v[:1]))
    return out


def old_accepts(got, ref64, dt):
    ref = ref64.to(DT[dt]).float()
    err = float((got.float() - ref).abs().max())
    return math.isfinite(err) and err <= OLD_TOL[dt] * max(float(ref.abs().max()), 1e-6)
