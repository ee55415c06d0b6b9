"""Shapes, guarded buffers and fp64 references of the graph kernels for 65..128 objects (csrc/graph_long.hip).

Importable without a GPU.  In the manner of gemm_edge_cases.py / attention_cases.py every tensor a kernel touches is a
contiguous window inside a larger buffer: inputs sit in a moat of NaNs (a load past the tensor poisons the result), outputs
in a band of sentinels that must be intact afterwards (a store past the tensor is seen even where nothing reads it).  The
graph entry points take dense contiguous tensors, so the window is a run of elements of a flat buffer, not a strided view.

The references are closed forms or autograd in fp64 on the operands AS STORED (bf16 inputs are rounded first and the
reference consumes the rounded values).  Tolerances live in the tests and are the ones the 64-object kernels are held to.
"""
import torch

NS = (65, 72, 100, 127, 128)  # one past the short kernels; 8 beyond a half; the 100-box features; odd; the largest
BS = (2, 9)                   # 9: more than one group of eight samples (the bf16 aggregate deals samples to XCDs in eights)
HS = (64, 96, 200)            # one column block; a ragged second block; four blocks, the last ragged and H % 16 != 0
LEAD, MOAT = 64, 4096         # elements in front of / behind a window (LEAD * itemsize keeps 16-byte alignment)
SENTINEL = -1234.0
F32, BF16 = torch.float32, torch.bfloat16
AGG_PLAIN, AGG_TRANSPOSE, AGG_SYMMETRIZE = 0, 1, 2


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Flat:
    """a contiguous tensor of ``shape`` inside a flat buffer of LEAD + numel + MOAT elements filled with ``fill``"""

    def __init__(self, shape, dtype, device, fill):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((LEAD + n + MOAT,), fill, dtype=dtype, device=device)
        self.view = self.buf[LEAD:LEAD + n].view(*shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0
        self.pristine = None

    def seal(self):
        self.pristine = self.buf.clone()
        return self

    def untouched_outside(self):
        cur = self.buf.clone()
        cur[LEAD:LEAD + self.n] = self.pristine[LEAD:LEAD + self.n]
        return torch.equal(_ints(cur), _ints(self.pristine))


def moated(value, device):
    """``value`` (CPU) as a device tensor inside a moat of NaNs (integers: a huge index)"""
    fill = float("nan") if value.is_floating_point() else 2 ** 30
    f = Flat(tuple(value.shape), value.dtype, device, fill)
    f.view.copy_(value)
    return f.view


def banded(shape, dtype, device, init=None):
    """an output window in a band of sentinels; the window itself starts as sentinels too (or ``init``, CPU)"""
    f = Flat(tuple(shape), dtype, device, SENTINEL if dtype.is_floating_point else -77)
    if init is not None:
        f.view.copy_(init)
    return f.seal()


def randn(shape, seed, dtype=F32, scale=1.0):
    """(values as stored, CPU; the same in fp64)"""
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)
    return x, x.double()


# ---------------------------------------------------------------------------------------------------- aggregate
def agg_matrix(a64, mode):
    return {AGG_PLAIN: a64, AGG_TRANSPOSE: a64.transpose(1, 2), AGG_SYMMETRIZE: a64 + a64.transpose(1, 2)}[mode]


def aggregate_ref(a64, x64, mode=AGG_PLAIN, scale=1.0, eps=None, self_w=0.0, base64=None):
    """[base +] self_w x + scale (1 + eps) M' x in fp64"""
    out = scale * (1.0 + (0.0 if eps is None else eps)) * (agg_matrix(a64, mode) @ x64) + self_w * x64
    return out if base64 is None else out + base64


def upper_only(B, N, seed):
    """an adjacency whose only non-zero entries sit in rows >= 64 AND columns >= 64: a kernel that stops at 64 neighbours
    or 64 output rows returns zeros, not nearly right numbers"""
    a = torch.zeros(B, N, N)
    a[:, 64:, 64:] = torch.randn(B, N - 64, N - 64, generator=torch.Generator().manual_seed(seed))
    return a


# ---------------------------------------------------------------------------------------------------- adj_regen
TIES = ((10, 70), (63, 64), (64, -1))   # (lower row, upper row) of exact ties at the column maximum; -1: row N - 1
PLANTED = (0, 63, 64, -1)               # rows that hold a planted unique column maximum


def regen_scores(B, N, H, seed):
    """S = x x^T (fp32, CPU) of sample-wise random x, with planted column maxima and exact ties.
    Returns (S, planted) with planted = [(sample, column, expected arg-max row)]."""
    x = torch.randn(B, N, H, generator=torch.Generator().manual_seed(seed)).double()
    S = (x @ x.transpose(1, 2)).float()
    planted = []
    col = 1
    for k, r in enumerate(PLANTED):       # sample 0: unique maxima
        r = r % N
        S[0, r, col] = S[0, :, col].max() + 1.0 + k
        planted.append((0, col, r))
        col += 7
    for lo, hi in TIES:                   # sample 1: ties, the lower row must win
        lo, hi = sorted((lo, N - 1 if hi < 0 else min(hi, N - 1)))  # (N = 65: 70 -> 64)
        m = S[1, :, col].max() + 2.0
        S[1, lo, col] = m
        S[1, hi, col] = m
        planted.append((1, col, lo))
        col += 7
    return S, planted


def regen_ref(S32, g32=None):
    """(adj, arg-max, dS) of src/module/graph_generative_modeling.py:225-228 in fp64 autograd on the fp32 scores"""
    Sr = S32.double().requires_grad_(True)
    mx, am = Sr.max(dim=1)
    s = torch.sigmoid(Sr / mx.unsqueeze(-1))
    ref = s.triu(1) + s.tril(-1)
    dS = None
    if g32 is not None:
        (ref * g32.double()).sum().backward()
        dS = Sr.grad
    return ref.detach(), am, dS


# ---------------------------------------------------------------------------------------------------- gat_att
def gat_inputs(B, N, seed):
    """s [B*N, 2], adj [B, N, N] (0 / 1 with special rows), d_att [B, N, N], all fp32 CPU.
    sample 0: row 3 sees only neighbours >= 64, row 5 is fully masked (uniform 1 / N), row min(70, N - 1) sees only
    neighbours < 64;
    sample 1: no masked entry at all; further samples: random masks."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B * N, 2, generator=g)
    adj = (torch.rand(B, N, N, generator=g) < 0.4).float()
    adj[0, 3, :64] = 0.0
    adj[0, 3, 64:] = 1.0
    adj[0, 5, :] = 0.0
    adj[0, min(70, N - 1), :] = 0.0
    adj[0, min(70, N - 1), :64] = 1.0
    adj[1] = 1.0
    d_att = torch.randn(B, N, N, generator=g)
    return s, adj, d_att


def gat_ref(s32, adj32, d_att32, alpha):
    """fp64 autograd restatement of src/module/gat.py:25-49 from the two per-node scalars: (att, ds [B*N, 2])"""
    B, N, _ = adj32.shape
    s = s32.double().requires_grad_(True)
    sv = s.view(B, N, 2)
    e = sv[:, :, 0].unsqueeze(2) + sv[:, :, 1].unsqueeze(1)  # [B, N, N]: self i, neighbour j
    e = torch.nn.functional.leaky_relu(e, alpha)
    e = e.masked_fill(adj32 == 0, -9e15)
    att = torch.softmax(e, dim=-1)
    (att * d_att32.double()).sum().backward()
    return att.detach(), s.grad


# ---------------------------------------------------------------------------------------------------- whole passes
PASS_KINDS = ["rel", "node", "rel", "node", "plain"]
PASS_CONFIGS = {"gcn100": ("GCN", 100), "gin72": ("GIN", 72), "gcn128": ("GCN", 128)}
PASS_WEIGHTS = ["encoder_adj.0.weight", "node_fc.0.weight", "fusion_fc.0.weight", "logit_fc.3.weight"]


# ---------------------------------------------------------------------------------------------------- GIN's eps in bf16
# d eps = sum_{b,i,j} A_ij (d_hin x^T)_ij is ONE cancelling sum.  Operands that each carry a relative error rho move it by at
# most rho * M, M = sum |A_ij (d_hin x^T)_ij| its mass, whatever its value.  test_model_gpu's rule for bf16 -- 3 % of the
# generator's largest eps gradient -- was set at gen_gin36, whose largest eps gradient (179.857) is 0.01436 of its mass
# (12 523.7, fp64 oracle): the rule grants rho = 0.03 * 0.01436 = 4.3e-4 of the mass, a ninth of one bf16 rounding (2^-8)
# per term.  A fixture whose sum cancels harder has a larger mass per unit of value (gen_gin72: 11.43 on 8 744.4 and 2.78 on
# 2 002.1, ratios 0.0013 and 0.0014, ten times harder), so there the same rho is a larger share of the value; the bound is
# stated in the mass, with the mass taken from the fp64 oracle, never from the kernels.
EPS_RHO = 0.03 * 0.01436


def gin_eps_mass(tag, g):
    """{eps parameter name: mass of its gradient sum} of a GIN fixture, by the fp64 oracle: eps is handed over as a
    [B, N, N] tensor of equal entries, whose gradient holds the (b, i, j) terms of the sum"""
    from oracle import shapes, xggm_oracle as O
    from xggm_amd import synth
    from helpers import probe, seeded_params
    kind, H, N, B = str(g["kind"]), int(g["H"]), int(g["N"]), int(g["B"])
    nl, seed = int(g["n_layers"]), int(g["seed"])
    P = {k: v.double() for k, v in seeded_params(shapes.generator_shapes(kind, H, nl), seed).items()}
    E = {k: (P[k].reshape(()) * torch.ones(B, N, N, dtype=torch.float64)).requires_grad_(True) for k in P if k.endswith("eps")}
    P.update(E)
    xn, an = synth.generator_inputs(tag, kind, B, N, H, seed)
    xo, ao = O.GENERATORS[kind](P, "generator.", torch.from_numpy(xn).double(), torch.from_numpy(an).double(), nl)
    ((xo * probe("xo", xo.shape, seed).double()).sum() + (ao * probe("ao", ao.shape, seed).double()).sum()).backward()
    return {k: float(e.grad.abs().sum()) for k, e in E.items()}


# ---------------------------------------------------------------------------------------------------- near-ties of the column maximum
# The regeneration divides row i of S = x x^T by max_r S[r][i], and the gradient of that maximum goes to ONE row, the
# arg-max: as a function of x the gradient is discontinuous where two rows tie.  With bf16 storage the generator's output x
# is rounded before S is taken: each component moves by at most 2^-9 relative (round to nearest), so to first order
# |d (x_r . x_j)| <= 2 * 2^-9 |x_r| |x_j| (Cauchy-Schwarz), and the two largest entries r, r' of column j may change order
# whenever     S[r][j] - S[r'][j] <= 2 * 2^-9 |x_j| (|x_r| + |x_r'|).
# For such a column either row is the arg-max of a correctly rounded computation and either gradient is a right answer.
# gen_gat128 (256 columns of 128 entries) has such columns -- its closest pair is 3.5e-5 of the maximum apart, sixty times
# below that threshold -- and an fp64 restatement of the generator that only rounds where the bf16 path stores (no kernel
# involved) flips one of them: dx then differs from the fixture by 7.1e-2, with the flip taken back by 6e-3.  So the bf16
# comparison of dx is made against the ADMISSIBLE references: the fp64 oracle with, in every near-tied column, the
# arg-max row that explains the result better (greedy over the columns, closest pair first).  The tolerance stays the
# inherited one, the fp32 comparison stays against the fixture itself, and so does everything else in bf16.  (Only the two
# largest entries of a column are considered; a third within the threshold is not.)
TIE_RHO = 2.0 ** -9


def regen_adj_at(x, idx):
    """oracle.regen_adj with the column maximum read at the given rows ``idx`` [B, N] (its own arg-max: the same values and
    gradient): src/module/graph_generative_modeling.py:225-228"""
    s = torch.bmm(x, x.transpose(1, 2))
    s = torch.sigmoid(s / s.gather(1, idx.unsqueeze(1)).squeeze(1).unsqueeze(-1))
    return s.triu(1) + s.tril(-1)


class GatTieRefs:
    """the fp64 oracle of a one-layer GAT generator fixture with a choice of arg-max rows: ``dx(idx)``; ``idx0`` the oracle's
    own arg-max, ``near`` the near-tied columns [(sample, column)] closest pair first, ``second`` the runner-up rows"""

    def __init__(self, tag, g):
        from oracle import shapes, xggm_oracle as O
        from xggm_amd import synth
        from helpers import probe, seeded_params
        kind, H, N, B = str(g["kind"]), int(g["H"]), int(g["N"]), int(g["B"])
        nl, seed = int(g["n_layers"]), int(g["seed"])
        assert kind == "GAT" and nl == 1
        P = {k: v.double() for k, v in seeded_params(shapes.generator_shapes(kind, H, nl), seed).items()}
        xn, an = synth.generator_inputs(tag, kind, B, N, H, seed)
        self.x = torch.from_numpy(xn).double().requires_grad_(True)
        self.xo = O.gat(P, "generator.gnn_layers.0.", self.x, torch.from_numpy(an).double(), 2)
        self.leaf = self.xo.detach().requires_grad_(True)
        self.p_xo = probe("xo", self.xo.shape, seed).double()
        self.p_ao = probe("ao", (B, N, N), seed).double()
        S = torch.bmm(self.leaf.detach(), self.leaf.detach().transpose(1, 2))
        top = S.topk(2, dim=1)
        self.idx0, self.second = top.indices[:, 0], top.indices[:, 1]
        gap = top.values[:, 0] - top.values[:, 1]
        nrm = self.leaf.detach().norm(dim=-1)
        thr = 2 * TIE_RHO * nrm * (nrm.gather(1, self.idx0) + nrm.gather(1, self.second))
        self.min_gap = float((gap / top.values[:, 0].abs()).min())
        near = (gap <= thr).nonzero().tolist()
        self.near = sorted(((b, j) for b, j in near), key=lambda t: float(gap[t[0], t[1]]))

    def dx(self, idx):
        ao = regen_adj_at(self.leaf, idx)
        d_xo = torch.autograd.grad((ao * self.p_ao).sum(), self.leaf)[0] + self.p_xo
        return torch.autograd.grad(self.xo, self.x, d_xo, retain_graph=True)[0]

    def admissible_err(self, got):
        """(smallest rel_err of ``got`` against an admissible reference found greedily, columns flipped)"""
        from helpers import rel_err
        idx, flipped = self.idx0.clone(), []
        cur = rel_err(got, self.dx(idx))
        for b, j in self.near:
            t = idx.clone()
            t[b, j] = self.second[b, j]
            e = rel_err(got, self.dx(t))
            if e < cur:
                cur, idx = e, t
                flipped.append((b, j))
        return cur, flipped
