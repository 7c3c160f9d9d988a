"""GenCast's mesh transformer on the device: ``utils/sparse_transformer.py::Transformer``.

The reference's processor between the norm-conditioned encoder and decoder (``weathernext1_gen/denoiser.py:330-335``)
is a stack of ``num_layers`` blocks over the mesh nodes ``x [B, N, d_model]``::

    x += mha_final(attn(cond_b(LN(x))))                   (mha_proj_q / _k / _v without bias)
    x += ffw_down(gelu(ffw_up(cond_b'(LN(x)))))           (gelu = jax.nn.gelu's default, the tanh form)
    out = cond_final(LN(x))

with ``cond(y) = y * (1 + s_b) + o_b``, ``[s_b | o_b] = c_b @ W + b`` (``dense.LinearNormConditioning``) and the
attention restricted to ``mask = adj ** attention_k_hop`` -- a scipy MATRIX power of the mesh adjacency with self
edges, rows = senders: query t attends key T iff ``mask[t, T]``.  ``attention_type`` ``mha``, ``triblockdiag_mha`` and
``splash_mha`` compute that same function (their TPU tiling arguments are accepted and ignored, as ``deep_gnn.py``
does with its remat / sharding arguments).

On the MI355X (all arithmetic in libgcast_hip.so):
  * the mask is built once per graph and cached on the index bytes; the nodes are renumbered into an internal order
    with locality (a 3-D Morton order when node positions are given, else the reverse Cuthill-McKee order of the
    graph), cut into 64-row tiles, and every (query tile, key tile) pair the mask touches gets a 64 x 64 bitmask --
    the CSR tile list that ``gc_attention`` walks (csrc/attention.inc);
  * the Linear layers are ``gc_rowmlp`` GC_MODE_LINEAR launches (Q / K / V; mha_final with the residual as the
    direct addend; ffw_up as four 512-column launches into a 2048-wide buffer; ffw_down over K = 2048 plus residual
    and bias); the conditioning vectors are LINEAR launches over the [B, C] conditioning rows (the + 1 folded into
    the bias, as in ``conditioned.py``); LayerNorm + conditioning and gelu are the small kernels of attention.inc;
  * inputs are gathered into the internal order and the output scattered back (``gc_permute_rows``): the block is
    permutation-equivariant, so the caller's node order is unaffected.
"""
import ctypes
import hashlib
from typing import Mapping, Optional

import numpy as np
import torch
from scipy import sparse
from scipy.sparse import csgraph

from graphcast_amd import _native as nat
from graphcast_amd import launch
from graphcast_amd import packing

D = packing.LATENT
TILE = 64
HEADS, KEY, HIDDEN = 4, 128, 2048

_MASKS = {}          # index bytes -> (mask, order, tiles): built once per graph (cf. DeepGNN._edges_of)


# ---------------------------------------------------------------------------------------------------- host structure
def adjacency(n, senders, receivers):
  """Boolean [n, n] csr: adj[s, r] = True for every edge, plus self edges (weathernext1_gen/transformer.py)."""
  s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
  adj = sparse.csr_matrix((np.ones(len(s), np.bool_), (s, r)), shape=(n, n))
  adj = adj + sparse.identity(n, dtype=np.bool_, format="csr")
  adj = sparse.csr_matrix(adj, dtype=np.bool_)
  adj.sum_duplicates()
  return adj


def k_hop_mask(adj, k):
  """``adj ** k`` as the reference computes it (a scipy csr_matrix power: the MATRIX power), indices sorted."""
  m = sparse.csr_matrix(adj, dtype=np.bool_) ** int(k)
  m = sparse.csr_matrix(m, dtype=np.bool_)
  m.eliminate_zeros()
  m.sort_indices()
  return m


def morton_order(positions):
  """Nodes sorted by the 3-D Morton (Z-order) code of their positions (10 bits per axis)."""
  p = np.asarray(positions, np.float64)
  lo, hi = p.min(0), p.max(0)
  q = np.clip(((p - lo) / np.maximum(hi - lo, 1e-12) * 1023).astype(np.int64), 0, 1023)
  code = np.zeros(len(p), np.int64)
  for bit in range(10):
    for ax in range(3):
      code |= ((q[:, ax] >> bit) & 1) << (3 * bit + ax)
  return np.argsort(code, kind="stable")


def rcm_order(adj):
  """Reverse Cuthill-McKee order of the symmetrised graph (what icosahedral_mesh.get_permutation_to_banded uses)."""
  sym = sparse.csr_matrix(adj + adj.T, dtype=np.bool_)
  return np.asarray(csgraph.reverse_cuthill_mckee(sym, symmetric_mode=True), np.int64)


class Tiles:
  """The tiled mask in an internal node order: ``order[i]`` = caller node of internal row i; query tile i touches key
  tiles ``col[ptr[i]:ptr[i + 1]]``; ``bits[t, r]`` bit c = internal row 64 i + r may attend internal row
  64 col[t] + c."""

  def __init__(self, mask, order):
    n = mask.shape[0]
    self.n, self.order = n, np.asarray(order, np.int64)
    inv = np.empty(n, np.int64)
    inv[self.order] = np.arange(n)
    self.inverse = inv
    coo = mask.tocoo()
    r, c = inv[coo.row], inv[coo.col]
    n_t = (n + TILE - 1) // TILE
    key = (r // TILE) * n_t + (c // TILE)
    tiles, tid = np.unique(key, return_inverse=True)
    self.n_qtiles = n_t
    self.col = (tiles % n_t).astype(np.int32)
    qt = tiles // n_t
    self.ptr = np.zeros(n_t + 1, np.int32)
    np.add.at(self.ptr, qt + 1, 1)
    self.ptr = np.cumsum(self.ptr).astype(np.int32)
    words = tid * TILE + (r % TILE)
    bit = np.left_shift(np.uint64(1), (c % TILE).astype(np.uint64))
    o = np.argsort(words, kind="stable")
    words, bit = words[o], bit[o]
    starts = np.flatnonzero(np.r_[True, words[1:] != words[:-1]])
    self.bits = np.zeros(len(tiles) * TILE, np.uint64)
    self.bits[words[starts]] = np.add.reduceat(bit, starts)      # distinct bits of one word: sum == or
    self.mask_nnz = int(mask.nnz)

  @property
  def n_tiles(self):
    return len(self.col)

  def stats(self):
    """Key tiles per query tile, mask density inside the touched tiles, useful / tile-level products."""
    return dict(n=self.n, query_tiles=self.n_qtiles, tiles=self.n_tiles,
                tiles_per_query_tile=self.n_tiles / self.n_qtiles,
                density=self.mask_nnz / (self.n_tiles * TILE * TILE))


def tiles_for(n, senders, receivers, k, positions=None):
  """(mask, Tiles) of a graph, built once per index set (cached on the index bytes)."""
  s, r = np.ascontiguousarray(senders, np.int64), np.ascontiguousarray(receivers, np.int64)
  h = hashlib.sha256(s.tobytes() + b"|" + r.tobytes() + f"|{n}|{k}".encode())
  if positions is not None:
    h.update(np.ascontiguousarray(positions, np.float64).tobytes())
  key = h.hexdigest()
  if key not in _MASKS:
    adj = adjacency(n, s, r)
    mask = k_hop_mask(adj, k)
    order = morton_order(positions) if positions is not None else rcm_order(adj)
    _MASKS[key] = (mask, Tiles(mask, order))
  return _MASKS[key]


def adjacency_of_csr(adj):
  """senders / receivers of a boolean csr adjacency (self edges included: harmless, they are added anyway)."""
  coo = sparse.csr_matrix(adj).tocoo()
  return coo.row.astype(np.int64), coo.col.astype(np.int64)


def check_global_conditioning(cond):
  """The transformer is conditioned by ONE vector per batch element ([B, C]); per-node (spatial) norm conditioning
  is not built."""
  if len(cond.shape) != 2:
    raise NotImplementedError(f"only global norm conditioning [B, C] is built, got shape {tuple(cond.shape)} "
                              "(spatial norm conditioning is not)")


# ---------------------------------------------------------------------------------------------------- the device model
class _CondLayer:
  """One ``<name>/linear`` of dense.LinearNormConditioning: packed halves of w, biases with the + 1 folded in."""

  def __init__(self, params, key, kc, up, pack):
    w = np.asarray(params[key]["w"], np.float32)
    b = np.asarray(params[key]["b"], np.float32)
    if w.shape[1] != 2 * D:
      raise NotImplementedError(f"{key}: norm conditioning must produce 2 x {D} values, got {w.shape}")
    wp = np.zeros((kc, 2 * D), np.float32)
    wp[:w.shape[0]] = w
    self.w_scale, self.w_offset = pack(wp[:, :D]), pack(wp[:, D:])
    self.b_scale, self.b_offset = up(b[:D] + np.float32(1.0)), up(b[D:])


class Transformer(launch.LaunchBase):
  """``sparse_transformer.Transformer`` on the device.

  Same constructor arguments as the reference (``adj_mat``, ``attention_k_hop``, ``attention_type``, ``mask_type``,
  ``num_heads``, ``name``, the ``block_*`` tiling arguments and the ``_ModelConfig`` keywords ``num_layers``,
  ``d_model``, ``key_size``, ``value_size``, ``ffw_hidden``, ``activation``, ...) plus ``params=`` (the haiku tree:
  ``<prefix><name>/block_%02d/...`` and ``<prefix><name>/<name>_final_norm_conditioning/linear``; any prefix, e.g.
  ``mesh_transformer/~/``), ``device=``, ``precision=`` (``f16x3`` | ``f32``) and ``node_positions=`` (optional
  [N, 3]: the internal order then is their Morton order).  Called as ``(x [B, N, 512], global_norm_conditioning
  [B, C])`` with float32 tensors on ``device``; returns [B, N, 512] in the caller's node order."""

  def __init__(self, adj_mat, attention_k_hop: int, attention_type: str, mask_type: Optional[str] = "full",
               num_heads: int = 1, name: Optional[str] = None, block_q=None, block_kv=None, block_kv_compute=None,
               block_q_dkv=None, block_kv_dkv=None, block_kv_dkv_compute=None, *, params: Mapping = None,
               device="cuda:0", precision: Optional[str] = None, node_positions=None, num_layers: int = None,
               d_model: int = None, key_size: Optional[int] = None, value_size: Optional[int] = None,
               activation: str = "gelu", ffw_hidden: Optional[int] = None, upcast_attn_to_fp32: bool = False,
               dtype=None, **init_scales):
    del block_q, block_kv, block_kv_compute, block_q_dkv, block_kv_dkv, block_kv_dkv_compute, upcast_attn_to_fp32
    if attention_type not in ("mha", "triblockdiag_mha", "splash_mha"):
      raise ValueError(f"Unsupported attention type: {attention_type}")
    if mask_type not in (None, "full", "lazy"):
      raise ValueError(f"Unsupported mask type: {mask_type}")
    bad = set(init_scales) - {"ffw_winit_mult", "ffw_winit_final_mult", "attn_winit_mult", "attn_winit_final_mult"}
    if bad:
      raise TypeError(f"unexpected arguments {sorted(bad)}")
    if num_layers is None or d_model is None:
      raise TypeError("num_layers and d_model are required (sparse_transformer._ModelConfig)")
    ffw_hidden = 4 * d_model if ffw_hidden is None else ffw_hidden
    if d_model % num_heads:
      raise ValueError("num_heads has to divide d_model exactly")
    key_size = d_model // num_heads if key_size is None else key_size
    value_size = d_model // num_heads if value_size is None else value_size
    if d_model != D or num_heads != HEADS or key_size != KEY or value_size != KEY:
      raise NotImplementedError(f"the device transformer is built for d_model {D} = {HEADS} heads x {KEY} (GenCast's "
                                f"published shape), got d_model {d_model}, {num_heads} heads of {key_size} / {value_size}")
    if ffw_hidden != HIDDEN:
      raise NotImplementedError(f"ffw_hidden must be {HIDDEN} (GenCast's published shape), got {ffw_hidden}")
    if activation != "gelu":
      raise NotImplementedError(f"activation must be 'gelu' (GenCast's), got {activation!r}")
    dname = str(getattr(dtype, "name", getattr(dtype, "__name__", dtype))).replace("torch.", "")
    if dtype is not None and dname != "float32":
      raise NotImplementedError("only float32 activations are built (no bf16 tier for the transformer)")
    if params is None:
      raise ValueError("params= (the haiku parameter tree) is required")
    self.name = name or "transformer"
    self.num_layers, self.k_hop = int(num_layers), int(attention_k_hop)
    self.dev = torch.device(device)
    self.lib = nat.lib()
    precision = precision or launch.DEFAULT_PRECISION
    if precision not in ("f16x3", "f32"):
      raise NotImplementedError(f"precision must be 'f16x3' or 'f32', got {precision!r}")
    self.precision, self.prec = precision, nat.PRECISIONS[precision]
    self.half = self.prec == nat.PREC_F16X3
    self.scratch, self.onepass, self.check_all_rows = None, False, True
    self.range_flag = torch.zeros((1,), dtype=torch.int32, device=self.dev) if self.half else None
    self._keep = []

    # ---- mask, internal order, tiles
    adj = sparse.csr_matrix(adj_mat)
    if adj.shape[0] != adj.shape[1]:
      raise ValueError(f"adj_mat must be square, got {adj.shape}")
    self.n = adj.shape[0]
    s, r = adjacency_of_csr(adj)
    self.mask, self.tiles = tiles_for(self.n, s, r, self.k_hop, node_positions)
    up = lambda a, dt=None: self._up(a, dt or np.asarray(a).dtype)
    self.t_ptr, self.t_col = up(self.tiles.ptr), up(self.tiles.col)
    self.t_bits = up(self.tiles.bits.view(np.int64))
    self.order = up(self.tiles.order.astype(np.int32))         # internal row i <- caller node order[i]
    self.inverse = up(self.tiles.inverse.astype(np.int32))     # caller node j <- internal row inverse[j]

    # ---- parameters
    prefix = self._prefix(params)
    self.prefix = prefix
    c_cond = np.asarray(params[f"{prefix}{self.name}_final_norm_conditioning/linear"]["w"]).shape[0]
    self.c_cond, self.kc = c_cond, packing.round_up(c_cond, packing.K_CHUNK)
    pack = self._pack
    cond_pack = lambda w: self._pack(w)
    upf = lambda a: self._up(np.asarray(a, np.float32))
    self.layers = []
    for i in range(self.num_layers):
      blk = f"{prefix}block_{i:02d}/"
      get = lambda mod, leaf: np.asarray(params[blk + mod][leaf], np.float32)
      for mod, shape in (("mha_proj_q", (D, D)), ("mha_proj_k", (D, D)), ("mha_proj_v", (D, D)),
                         ("mha_final", (D, D)), ("ffw_up", (D, HIDDEN)), ("ffw_down", (HIDDEN, D))):
        if blk + mod not in params or get(mod, "w").shape != shape:
          raise ValueError(f"params: {blk + mod}/w must be {shape}")
        if mod.startswith("mha_proj") and "b" in params[blk + mod]:
          raise ValueError(f"params: {blk + mod} has a bias (the reference's has none)")
      w_up = get("ffw_up", "w")
      self.layers.append(dict(
          q=pack(get("mha_proj_q", "w")), k=pack(get("mha_proj_k", "w")), v=pack(get("mha_proj_v", "w")),
          f=pack(get("mha_final", "w")), fb=upf(get("mha_final", "b")),
          up=[pack(w_up[:, j * D:(j + 1) * D]) for j in range(HIDDEN // D)],
          upb=[upf(get("ffw_up", "b")[j * D:(j + 1) * D]) for j in range(HIDDEN // D)],
          down=pack(get("ffw_down", "w")), downb=upf(get("ffw_down", "b")),
          c0=_CondLayer(params, f"{blk}block_{i:02d}_norm_conditioning/linear", self.kc, upf, cond_pack),
          c1=_CondLayer(params, f"{blk}block_{i:02d}_norm_conditioning_1/linear", self.kc, upf, cond_pack)))
    self.final = _CondLayer(params, f"{prefix}{self.name}_final_norm_conditioning/linear", self.kc, upf, cond_pack)
    self._bufs = {}

  def _prefix(self, params):
    tail = f"{self.name}/block_00/mha_proj_q"
    hits = [k for k in params if k == tail or k.endswith("/" + tail)]
    if self.num_layers == 0:
      hits = [k[:-len("_final_norm_conditioning/linear")] for k in params
              if k.endswith(f"{self.name}_final_norm_conditioning/linear")]
      return hits[0][:-len(self.name)] + self.name + "/" if len(hits) == 1 else self.name + "/"
    if len(hits) != 1:
      raise ValueError(f"params: expected exactly one module '.../{tail}', found {hits}")
    return hits[0][:-len("block_00/mha_proj_q")]

  def _pack(self, w):
    """One Linear's w [K, 512] packed as a layer-1 matrix of this precision (the image launch._Mlp makes)."""
    k = w.shape[0]
    holder = {"x_mlp/~/linear_0": {"w": w, "b": np.zeros(D, np.float32)},
              "x_mlp/~/linear_1": {"w": np.zeros((D, D), np.float32), "b": np.zeros(D, np.float32)}}
    assert k % packing.K_CHUNK == 0, k
    return launch._Mlp(holder, "x", self.dev, prec=self.prec).w1

  # -------------------------------------------------------------------------------------------------- buffers
  def _buffers(self, batch):
    if batch not in self._bufs:
      rows = batch * self.n
      new = lambda cols=D: torch.empty((rows, cols), dtype=torch.float32, device=self.dev)
      self._bufs = {batch: dict(xa=new(), xb=new(), h=new(), q=new(), k=new(), v=new(), att=new(),
                                u=new(HIDDEN), cond=torch.zeros((batch, self.kc), dtype=torch.float32,
                                                                 device=self.dev))}
    return self._bufs[batch]

  # -------------------------------------------------------------------------------------------------- launches
  def _rowmlp(self, ds):
    nat.check(self.lib.gc_rowmlp(ctypes.byref(ds), self._stream_ptr()), "gc_rowmlp")

  def _linear(self, rows, a0, w, out, k0=D, d=None, b1=None, out_ptr=None, ldo=None):
    self._rowmlp(self._desc(nat.MODE_LINEAR, rows, a0=a0, k0=k0, w1p=w, d=d, b1=b1, out=out, out_ptr=out_ptr,
                            ldo=ldo))

  def _cond_vectors(self, c: _CondLayer, cond_rows, batch):
    scale = torch.empty((batch, D), dtype=torch.float32, device=self.dev)
    offset = torch.empty((batch, D), dtype=torch.float32, device=self.dev)
    self._linear(batch, cond_rows, c.w_scale, scale, k0=self.kc, b1=c.b_scale)
    self._linear(batch, cond_rows, c.w_offset, offset, k0=self.kc, b1=c.b_offset)
    return scale, offset

  def _ln_cond(self, x, so, out):
    nat.check(self.lib.gc_ln_cond_rows(x.shape[0], self.n, x.data_ptr(), so[0].data_ptr(), so[1].data_ptr(),
                                       out.data_ptr(), self._stream_ptr()), "gc_ln_cond_rows")

  def attention(self, q, k, v, out, batch):
    """gc_attention over [batch * n, 512] rows in the internal order."""
    nat.check(self.lib.gc_attention(
        self.prec, batch, self.n, self.tiles.n_qtiles, self.t_ptr.data_ptr(), self.t_col.data_ptr(),
        self.t_bits.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), D, KEY ** -0.5, out.data_ptr(), D,
        nat.ptr(self.range_flag), self._stream_ptr()), "gc_attention")

  def _permute(self, idx, src, dst, batch):
    nat.check(self.lib.gc_permute_rows(self.n, batch, idx.data_ptr(), src.data_ptr(), self.n, D, dst.data_ptr(),
                                       self.n, D, self._stream_ptr()), "gc_permute_rows")

  def __call__(self, node_features: torch.Tensor, global_norm_conditioning: torch.Tensor, check_range=True):
    x, cond = node_features, global_norm_conditioning
    if (x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != self.n or x.shape[2] != D or x.device != self.dev):
      raise ValueError(f"node_features must be a float32 [B, {self.n}, {D}] tensor on {self.dev}")
    batch = x.shape[0]
    check_global_conditioning(cond)
    if (cond.dtype != torch.float32 or cond.dim() != 2 or cond.shape != (batch, self.c_cond)
        or cond.device != self.dev):
      raise ValueError(f"global_norm_conditioning must be a float32 [{batch}, {self.c_cond}] tensor on {self.dev}")
    x = x.contiguous()
    bf = self._buffers(batch)
    rows = batch * self.n
    with torch.cuda.device(self.dev):
      self._tile_queue().zero_()
      bf["cond"][:, :self.c_cond] = cond
      cr = bf["cond"]
      xa, xb, h = bf["xa"], bf["xb"], bf["h"]
      self._permute(self.order, x, xa, batch)
      for L in self.layers:
        so0, so1 = self._cond_vectors(L["c0"], cr, batch), self._cond_vectors(L["c1"], cr, batch)
        self._ln_cond(xa, so0, h)
        self._linear(rows, h, L["q"], bf["q"])
        self._linear(rows, h, L["k"], bf["k"])
        self._linear(rows, h, L["v"], bf["v"])
        self.attention(bf["q"], bf["k"], bf["v"], bf["att"], batch)
        self._linear(rows, bf["att"], L["f"], xb, d=xa, b1=L["fb"])
        self._ln_cond(xb, so1, h)
        u = bf["u"]
        for j in range(HIDDEN // D):
          self._linear(rows, h, L["up"][j], None, b1=L["upb"][j], out_ptr=u.data_ptr() + 4 * j * D, ldo=HIDDEN)
        nat.check(self.lib.gc_gelu_rows(rows * HIDDEN, u.data_ptr(), self._stream_ptr()), "gc_gelu_rows")
        self._linear(rows, u, L["down"], xa, k0=HIDDEN, d=xb, b1=L["downb"])
      self._ln_cond(xa, self._cond_vectors(self.final, cr, batch), h)
      y = torch.empty_like(x)
      self._permute(self.inverse, h, y, batch)
    if check_range:
      self.check_range()
    return y
