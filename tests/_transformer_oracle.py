"""fp64 numpy restatement of GenCast's mesh transformer (utils/sparse_transformer.py Transformer / Block / mha with
utils/dense.py LinearNormConditioning), checked against tests/golden/transformer512.npz (the reference executed) on
the CPU and used by the GPU tests as the yardstick at sizes the fixture cannot hold.

Attention is evaluated sparsely (per query row over its allowed keys only), which is the same function as the
reference's dense masked softmax: the masked logits there are -1e30, whose exponentials are exactly 0."""
import numpy as np
from scipy import sparse

D, HEADS, KEY = 512, 4, 128
EPS = 1e-5


def k_hop_mask(n, senders, receivers, k):
  """adj ** k with adj[s, r] = True plus self edges (weathernext1_gen/transformer.py, sparse_transformer.py)."""
  adj = sparse.csr_matrix((np.ones(len(senders), np.bool_), (np.asarray(senders), np.asarray(receivers))),
                          shape=(n, n)) + sparse.identity(n, dtype=np.bool_, format="csr")
  adj = sparse.csr_matrix(adj, dtype=np.bool_)
  m = adj ** k
  m.sort_indices()
  return m


def _ln(x):
  mu = x.mean(-1, keepdims=True)
  var = np.square(x - mu).mean(-1, keepdims=True)
  return (x - mu) / np.sqrt(var + EPS)


def _cond(params, key, y, cond):
  p = params[key]
  so = cond @ np.asarray(p["w"], np.float64) + np.asarray(p["b"], np.float64)     # [B, 2D]
  return y * (1.0 + so[:, None, :D]) + so[:, None, D:]


def gelu(x):
  return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def attention(q, k, v, mask, rows=None, chunk=256):
  """q [B, R, D] for the query rows `rows` (all when None), k / v [B, N, D]; mask csr [N, N]."""
  b = q.shape[0]
  rows = np.arange(mask.shape[0]) if rows is None else np.asarray(rows)
  out = np.empty(q.shape, np.float64)
  for c0 in range(0, len(rows), chunk):
    rr = rows[c0:c0 + chunk]
    sub = mask[rr]
    deg = np.diff(sub.indptr)
    t = np.repeat(np.arange(len(rr)), deg)
    cols = sub.indices
    for bb in range(b):
      qh = q[bb, c0:c0 + chunk].reshape(len(rr), HEADS, KEY)
      kh = k[bb, cols].reshape(len(cols), HEADS, KEY)
      vh = v[bb, cols].reshape(len(cols), HEADS, KEY)
      logit = np.einsum("ehd,ehd->eh", qh[t], kh) * KEY ** -0.5
      mx = np.full((len(rr), HEADS), -np.inf)
      np.maximum.at(mx, t, logit)
      e = np.exp(logit - mx[t])
      den = np.zeros((len(rr), HEADS))
      np.add.at(den, t, e)
      num = np.zeros((len(rr), HEADS, KEY))
      np.add.at(num, t, e[:, :, None] * vh)
      out[bb, c0:c0 + chunk] = (num / den[:, :, None]).reshape(len(rr), D)
  return out


def block(params, prefix, i, mask, x, cond, rows=None):
  """One block_%02d: x [B, N, D] -> the block's output at `rows` (all when None)."""
  blk = f"{prefix}block_{i:02d}/"
  w = lambda name: np.asarray(params[blk + name]["w"], np.float64)
  bias = lambda name: np.asarray(params[blk + name]["b"], np.float64)
  c0 = f"{blk}block_{i:02d}_norm_conditioning/linear"
  c1 = f"{blk}block_{i:02d}_norm_conditioning_1/linear"
  h = _cond(params, c0, _ln(x), cond)
  q_rows = h if rows is None else h[:, rows]
  att = attention(q_rows @ w("mha_proj_q"), h @ w("mha_proj_k"), h @ w("mha_proj_v"), mask, rows)
  x1 = (x if rows is None else x[:, rows]) + att @ w("mha_final") + bias("mha_final")
  h1 = _cond(params, c1, _ln(x1), cond)
  return x1 + gelu(h1 @ w("ffw_up") + bias("ffw_up")) @ w("ffw_down") + bias("ffw_down")


def forward(params, mask, x, cond, num_layers, prefix="transformer/", name="transformer", rows=None):
  """Transformer(x [B, N, D], global_norm_conditioning [B, C]) in float64; `rows` restricts the LAST layer and the final
  conditioning to those rows."""
  x = np.asarray(x, np.float64)
  cond = np.asarray(cond, np.float64)
  for i in range(num_layers):
    x = block(params, prefix, i, mask, x, cond, rows=rows if i == num_layers - 1 else None)
  return _cond(params, f"{prefix}{name}_final_norm_conditioning/linear", _ln(x), cond)
