"""Host references for the training-row tests: a numpy Philox4x32 (Salmon et al., SC'11 / Random123) that is checked against the
published known-answer vectors in tests/test_host_train.py, the keep mask include/gator_train.h documents for gator_t_dropout, the
provider of those masks to the oracle's and the recorded reference's dropout sites (DropSites), and
float64 torch-CPU forms of the fused dropout-on operations built on that mask, of both LayerNorm modes, the MGCN layer and one Adam step
(each checked on the host in tests/test_host_train.py), the error criterion the new GPU tests share, and the per-term quantities of the
oracle's face losses from which the kink margins are measured.  Nothing here calls the library under test."""
import numpy as np
import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
DEVICE_ROUNDS = 7                       # GATOR_PHILOX_ROUNDS of gator_amd/csrc/train_ops.hip
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """counter [n, 4], key [n, 2] (or one row each) of 32-bit words -> [n, 4] uint32 words of the Philox4x32-`rounds` blocks."""
    c = np.atleast_2d(np.asarray(counter, dtype=np.uint64)) & _M32
    k = np.atleast_2d(np.asarray(key, dtype=np.uint64)) & _M32
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # 32 x 32 -> 64 bit products, exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _M32, (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), 1).astype(np.uint32)


def keep_threshold(rate):
    """uint32(rate * 2^32), saturated; the C ABI takes the rate as a float, so it is rounded to float32 first"""
    t = float(np.float32(rate)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def keep_mask(seed, offset, n, rate, step=0, rounds=DEVICE_ROUNDS):
    """uint8 [n]: element i is word i & 3 of the block with counter (i >> 2, offset + 2^32 * step) and key `seed`; kept when the
    word is >= the threshold."""
    n = int(n)
    quads = (n + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    off = (int(offset) + (int(step) << 32)) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty((quads, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = q & _M32, q >> np.uint64(32), off & 0xFFFFFFFF, off >> 32
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32(ctr, [[seed & 0xFFFFFFFF, seed >> 32]], rounds).reshape(-1)[:n]
    return (words >= np.uint32(keep_threshold(rate))).astype(np.uint8)


def keep_factor(seed, offset, shape, rate, step=0):
    """float64 torch tensor of `shape`: keep / (1 - rate) at the flat index of a contiguous tensor (ones when rate == 0)"""
    n = int(np.prod(shape))
    if rate <= 0.0:
        return torch.ones(shape, dtype=torch.float64)
    return torch.from_numpy(keep_mask(seed, offset, n, rate, step).astype(np.float64) / (1.0 - rate)).reshape(shape)


class DropSites:
    """The `drop` argument of the oracle's training forward (oracle/gator_oracle.py), and the forward hook of the recorded reference
    step (tools/gen_golden.py::train_drop_golden): every call with rate > 0 takes the next Philox offset, starting at `first_offset`,
    in the step word `step`, and multiplies by the host keep factor - per element at the flat index of the contiguous tensor
    (nn.Dropout), or one decision per sample broadcast over it (timm DropPath: shape (B, 1, ...), kept samples / (1 - rate)).  A call
    with rate == 0 draws nothing.  `log` holds one (site, kind, rate, shape, offset) per draw; `next_offset` is where the following
    step continues when the stream runs on."""

    def __init__(self, seed, first_offset=1, step=0):
        self.seed, self.next_offset, self.step, self.log = int(seed), int(first_offset), int(step), []

    def factor(self, site, shape, rate, per_sample=False):
        """float64 keep factor of one draw, broadcastable to `shape`; None when the site draws nothing"""
        rate = float(rate)
        if rate <= 0.0:
            return None
        shape = tuple(int(d) for d in shape)
        offset, self.next_offset = self.next_offset, self.next_offset + 1
        self.log.append((str(site), 'path' if per_sample else 'element', rate, shape, offset))
        if per_sample:
            keep = keep_mask(self.seed, offset, shape[0], rate, self.step).astype(np.float64) / (1.0 - rate)
            return torch.from_numpy(keep).reshape((shape[0],) + (1,) * (len(shape) - 1))
        return keep_factor(self.seed, offset, shape, rate, self.step)

    def __call__(self, site, x, rate, per_sample=False):
        f = self.factor(site, x.shape, rate, per_sample)
        return x if f is None else x * f.to(x.dtype)


PATH_FAMILIES = ('gat_attn_mgcn', 'gat_mlp', 'mdr_cross', 'mdr_mlp')


def path_families(log):
    """{family: [(rate, offset), ...]} of the per-sample draws of a DropSites log.  A block's DropPath module is called twice per
    forward (lib/models/GAT.py:38,42, MDR.py:66,68): its 1st, 3rd, ... call in the log is the attention branch (GAT: attention +
    MGCN; MDR: cross-attention), its 2nd, 4th, ... the MLP branch."""
    fam = {f: [] for f in PATH_FAMILIES}
    seen = {}
    for site, kind, rate, shape, offset in log:
        if kind != 'path':
            continue
        n = seen[site] = seen.get(site, 0) + 1
        gat = '.blocks.' in '.' + site                                  # GATBlock lives in GAT.blocks; CrossAttentionBlock is MDR.encoder*
        fam[('gat_attn_mgcn' if gat else 'mdr_cross') if n % 2 else ('gat_mlp' if gat else 'mdr_mlp')].append((rate, offset))
    return fam


def live_path_families(seed, log, B, step=0):
    """The families of path_families(log) in which at least one site keeps one of the B samples and drops another: masks under
    which per-sample DropPath differs from a per-batch or per-element decision and from none at all"""
    live = set()
    for f, draws in path_families(log).items():
        for rate, offset in draws:
            m = keep_mask(seed, offset, B, rate, step)
            if 0 < int(m.sum()) < B:
                live.add(f)
    return live


def attention_ref(q, k, v, heads, scale, keep):
    """q [B, T, H*D], k / v [B, Tk, H*D] float64; keep [B, H, T, Tk] (mask / (1 - rate)) -> [B, T, H*D]"""
    B, T, HD = q.shape
    D = HD // heads
    qq, kk, vv = [t.reshape(B, t.shape[1], heads, D).transpose(1, 2) for t in (q, k, v)]
    p = torch.softmax(scale * (qq @ kk.transpose(-2, -1)), -1) * keep
    return (p @ vv).transpose(1, 2).reshape(B, T, HD)


def attention_small_ref(qkv, bias, heads, scale, keep):
    """qkv [B, J, 3*H*D] laid out [B, J, 3, H, D], bias [H, J, J], keep [B, H, J, J] -> [B, J, H*D] head-major"""
    B, J, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    z = qkv.reshape(B, J, 3, heads, D).permute(2, 0, 3, 1, 4)
    p = torch.softmax(scale * (z[0] @ z[1].transpose(-2, -1)) + bias, -1) * keep
    return (p @ z[2]).transpose(1, 2).reshape(B, J, C)


def drop_fused_ref(x, res, gelu, elem_keep, path_keep):
    """res + path[b] * mask * act(x) / (1 - rate); elem_keep of x's shape, path_keep [B] (both already scaled), or None"""
    v = torch.nn.functional.gelu(x) if gelu else x
    if elem_keep is not None:
        v = v * elem_keep
    if path_keep is not None:
        v = v * path_keep.reshape([-1] + [1] * (x.dim() - 1))
    return v if res is None else res + v


def layernorm_ref(x, w, b, eps, mode):
    """float64 rows over the last dim.  mode 0: F.layer_norm (biased variance, eps inside the root); mode 1: w (x - mean) / (std + eps) + b
    with the unbiased std (lib/models/vanilla_transformer_encoder.py:31-34).  w, b may be None."""
    if mode == 0:
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)
    y = (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True, unbiased=True) + eps)
    if w is not None:
        y = w * y
    return y if b is None else y + b


def mgcn_ref(h0, h1, adj, M, bias):
    """include/gator_train.h: out = diag(adj) (M . h0) + (adj . (1 - I)) @ (M . h1) + bias; h0, h1 [B,J,C], adj [J,J], M [J,C], bias [C]"""
    eye = torch.eye(adj.shape[0], dtype=adj.dtype)
    return torch.diagonal(adj).reshape(1, -1, 1) * (M * h0) + (adj * (1.0 - eye)) @ (M * h1) + bias


def adam_step_ref(p, g, m, v, lr, b1, b2, eps, t):
    """One step of torch.optim.Adam's rule (no weight decay, no amsgrad) at step t >= 1 -> (p, m, v), float64"""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


def close_bound(ref64, tol=2e-5, noise32=None, scale=None):
    """(bound, scale) exactly as check_close forms them, for a test that must also cap the bound (the noise term must not make it vacuous)"""
    ref64 = ref64.detach().double()
    if scale is None:
        scale = max(1e-30, float(ref64.abs().max())) if ref64.numel() else 1.0
    bound = tol * scale
    if noise32 is not None:
        bound += 4.0 * float((noise32.detach().double() - ref64).abs().max())
    return bound, scale


def check_close(name, ours, ref64, tol=2e-5, noise32=None, verbose=True, scale=None):
    """|ours - ref64| <= tol * max|ref64| (+ 4 * max|noise32 - ref64| when the same operation in torch-CPU float32 is given).
    `scale` replaces max|ref64| where the caller has a reason (written down there).  Prints both terms; returns the achieved error."""
    ours = ours.detach().cpu().double() if torch.is_tensor(ours) else torch.as_tensor(ours, dtype=torch.float64)
    ref64 = ref64.detach().double()
    assert tuple(ours.shape) == tuple(ref64.shape), (name, tuple(ours.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(ours).all()), '%s: non-finite result' % name
    if scale is None:
        scale = max(1e-30, float(ref64.abs().max())) if ref64.numel() else 1.0
    err = float((ours - ref64).abs().max()) if ref64.numel() else 0.0
    bound = tol * scale
    if noise32 is not None:
        n32 = float((noise32.detach().double() - ref64).abs().max())
        bound += 4.0 * n32
        if verbose:
            print('%s: |ours - ref64| %.3e   |torch32 - ref64| %.3e   floor %.3e   bound %.3e' % (name, err, n32, tol * scale, bound))
    elif verbose:
        print('%s: |ours - ref64| %.3e   bound %.3e (scale %.3e)' % (name, err, bound, scale))
    assert err <= bound, '%s: error %.3e above the bound %.3e (scale %.3e)' % (name, err, bound, scale)
    return err


# ---- mesh losses: the per-term quantities of oracle.gator_oracle.normal_vector_loss / edge_length_loss, for the kink margins ----
TERM_CORNERS = ((0, 1), (0, 2), (1, 2))         # the two face corners each of the three terms of a face touches (both losses)


def normal_terms(coord_out, coord_gt, face):
    """signed cosines [B, 3, F] whose absolute values normal_vector_loss averages (same formula, same dtype as the input)"""
    F_ = torch.nn.functional
    face = torch.as_tensor(np.asarray(face)).long()
    nz = lambda v: F_.normalize(v, p=2, dim=2)
    normal_gt = nz(torch.cross(nz(coord_gt[:, face[:, 1]] - coord_gt[:, face[:, 0]]), nz(coord_gt[:, face[:, 2]] - coord_gt[:, face[:, 0]]), dim=2))
    return torch.stack([(nz(coord_out[:, face[:, b]] - coord_out[:, face[:, a]]) * normal_gt).sum(2) for a, b in TERM_CORNERS], 1)


def edge_terms(coord_out, coord_gt, face):
    """length residuals [B, 3, F] whose absolute values edge_length_loss averages"""
    face = torch.as_tensor(np.asarray(face)).long()
    d = lambda x, a, b: torch.sqrt(((x[:, face[:, a]] - x[:, face[:, b]]) ** 2).sum(2))
    return torch.stack([d(coord_out, a, b) - d(coord_gt, a, b) for a, b in TERM_CORNERS], 1)


def kink_exclusions(terms64, terms32, face, num_verts):
    """(excluded [B, V] bool, margin): |x| has a kink at 0, where a float32 evaluation may pick the other sign.  The margin is 8 x the
    largest float32 - float64 difference of a term; a vertex is excluded when a term it touches lies within the margin of 0 IN THE
    FLOAT64 REFERENCE (never judged from a device result)."""
    margin = 8.0 * float((terms32.double() - terms64).abs().max())
    near = (terms64.abs() < margin).numpy()                        # [B, 3, F]
    face = np.asarray(face).reshape(-1, 3)
    excl = np.zeros((terms64.shape[0], num_verts), bool)
    for t, corners in enumerate(TERM_CORNERS):
        b, f = np.nonzero(near[:, t])
        for c in corners:
            excl[b, face[f, c]] = True
    return excl, margin
