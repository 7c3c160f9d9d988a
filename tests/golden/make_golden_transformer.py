"""Generates tests/golden/transformer512.npz: GenCast's mesh transformer -- utils/sparse_transformer.py (Transformer,
Block, mha, triblockdiag_mha) and weathernext1_gen/transformer.py (MeshTransformer), with utils/dense.py
(LinearNormConditioning) -- executed UNMODIFIED on the numpy stand-ins of tests/golden/ref_shims, at the width the HIP
kernels are built for (d_model 512, 4 heads of 128, ffw_hidden 2048), for attention_type "mha" and
"triblockdiag_mha".  Also records the reference's banded mesh order (icosahedral_mesh.get_permutation_to_banded) at
M4 -- M6 as hashes.

Stand-ins added HERE for what the shims do not have (stated, not hidden):
  * jax.vmap (a Python loop over the mapped axis), jax.nn.softmax (over the last axis, max-shifted), jax.nn.gelu (jax's default, approximate=True: the tanh form),
    jax.custom_vjp (identity decorator), hk.initializers.VarianceScaling (parameters are installed, never drawn);
  * jax.experimental.pallas.ops.tpu.splash_attention: a module stub with splash_attention_mask.Mask /
    MultiHeadMask and BlockSizes -- imported by sparse_transformer.py, never executed here;
  * utils/sparse_transformer_utils.wrap_fn_for_upcast_downcast: its job is to run the softmax of BF16 activations
    in float32; on the float64 stand-ins it would ROUND to float32, so here it calls the function as it is.
Parameters are regenerated from a seed on both sides (tests/golden/transformer_case.py); the script asserts that the
seeded tree is exactly the one the reference asks for and stores the key set.

    python tests/golden/make_golden_transformer.py
"""
import hashlib
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "ref_shims"))
sys.path.insert(0, REF)

import typing                                                # noqa: E402
import typing_extensions                                     # noqa: E402
for _n in ("Required", "NotRequired"):
  if not hasattr(typing, _n):
    setattr(typing, _n, getattr(typing_extensions, _n))

import haiku as hk                                           # noqa: E402  (numpy stand-in)
import jax                                                   # noqa: E402  (numpy stand-in)
import weathernext.utils                                     # noqa: E402


def _install_stand_ins():
  def vmap(f, in_axes=0):
    def mapped(*args):
      axes = in_axes if isinstance(in_axes, (list, tuple)) else [in_axes] * len(args)
      size = next(np.shape(a)[ax] for a, ax in zip(args, axes) if ax is not None)
      outs = [f(*[a if ax is None else np.take(a, i, axis=ax) for a, ax in zip(args, axes)]) for i in range(size)]
      return np.stack(outs)
    return mapped

  def gelu(x, approximate=True):
    if not approximate:
      raise NotImplementedError("stand-in: jax.nn.gelu(approximate=True) only (the default)")
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))

  def softmax(x, axis=-1):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)

  jax.vmap = vmap
  jax.nn.gelu = staticmethod(gelu)
  jax.nn.softmax = staticmethod(softmax)
  jax.custom_vjp = lambda f, *a, **k: f
  hk.initializers.VarianceScaling = staticmethod(lambda *a, **k: None)

  exp = types.ModuleType("jax.experimental")
  pallas = types.ModuleType("jax.experimental.pallas")
  ops = types.ModuleType("jax.experimental.pallas.ops")
  tpu = types.ModuleType("jax.experimental.pallas.ops.tpu")
  splash = types.ModuleType("jax.experimental.pallas.ops.tpu.splash_attention")
  mask_mod = types.ModuleType("jax.experimental.pallas.ops.tpu.splash_attention.splash_attention_mask")

  class Mask:
    pass

  class MultiHeadMask(Mask):
    def __init__(self, masks):
      self.masks = masks

  mask_mod.Mask, mask_mod.MultiHeadMask = Mask, MultiHeadMask
  splash.splash_attention_mask = mask_mod
  splash.BlockSizes = lambda **k: k

  def make_splash_mha(*a, **k):
    raise NotImplementedError("stand-in: splash attention is not executed here")
  splash.make_splash_mha = make_splash_mha
  jax.experimental = exp
  exp.pallas, pallas.ops, ops.tpu, tpu.splash_attention = pallas, ops, tpu, splash
  for name, mod in (("jax.experimental", exp), ("jax.experimental.pallas", pallas),
                    ("jax.experimental.pallas.ops", ops), ("jax.experimental.pallas.ops.tpu", tpu),
                    ("jax.experimental.pallas.ops.tpu.splash_attention", splash),
                    ("jax.experimental.pallas.ops.tpu.splash_attention.splash_attention_mask", mask_mod)):
    sys.modules[name] = mod

  stu = types.ModuleType("weathernext.utils.sparse_transformer_utils")
  stu.wrap_fn_for_upcast_downcast = lambda inputs, fn, *a, **k: fn(inputs)
  sys.modules["weathernext.utils.sparse_transformer_utils"] = stu
  weathernext.utils.sparse_transformer_utils = stu


_install_stand_ins()
from weathernext.utils import icosahedral_mesh as ref_mesh     # noqa: E402
from weathernext.utils import sparse_transformer               # noqa: E402
from weathernext.utils import typed_graph                      # noqa: E402
from weathernext.weathernext1_gen import transformer as ref_transformer   # noqa: E402
from oracle import params as oparams                           # noqa: E402
from tests.golden import transformer_case as tc                # noqa: E402  (no reference imports there)

KW = dict(d_model=tc.D, num_layers=tc.LAYERS, num_heads=tc.HEADS, ffw_hidden=tc.HIDDEN, mask_type="full")


def _graph(n, s, r, x):
  return typed_graph.TypedGraph(
      context=typed_graph.Context(n_graph=np.array([1]), features=()),
      nodes={"mesh_nodes": typed_graph.NodeSet(n_node=np.array([n]), features=x)},
      edges={typed_graph.EdgeSetKey("mesh", ("mesh_nodes", "mesh_nodes")): typed_graph.EdgeSet(
          n_edge=np.array([len(s)]), indices=typed_graph.EdgesIndices(senders=s, receivers=r), features=())})


def _learn_keys(n, s, r, x, cond, wrapped):
  """The parameter tree the reference asks for (haiku stand-in with an init rng: every leaf it creates)."""
  store = {}
  with hk.running(store, init_rng=np.random.default_rng(0)) as st:
    if wrapped:
      ref_transformer.MeshTransformer(sparse_transformer.Transformer, dict(
          attention_k_hop=2, attention_type="mha", **KW), name="mesh_transformer")(_graph(n, s, r, x), cond)
    else:
      sparse_transformer.Transformer(_adj(n, s, r), attention_k_hop=2, attention_type="mha", **KW)(x, cond)
    created = st["created"]
  return {m: {leaf: shape for mm, leaf, shape in created if mm == m} for m in {c[0] for c in created}}


def _adj(n, s, r):
  """The reference's own adjacency (transformer.py: rows = senders, plus self edges)."""
  import warnings
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")            # (scipy's SparseEfficiencyWarning for the item assignment)
    return ref_transformer._get_adj_matrix_for_edge_set(_graph(n, s, r, np.zeros((n, 1, 1))), "mesh", add_self_edges=True)


def _run(n, s, r, k, att, x, cond, params):
  with hk.running(params):
    return np.asarray(sparse_transformer.Transformer(_adj(n, s, r), attention_k_hop=k, attention_type=att, **KW)(
        x, cond))


def banded_hashes():
  out = {}
  for level in (4, 5, 6):
    mesh = ref_mesh.get_hierarchy_of_triangular_meshes_for_sphere(splits=level)[-1]
    perm, _ = ref_mesh.get_permutation_to_banded(mesh)
    out[f"M{level}"] = dict(n=int(len(perm)), sha256=hashlib.sha256(np.asarray(perm, np.int64).tobytes()).hexdigest())
  return out


def main():
  out = dict(config=np.array([tc.D, tc.HEADS, tc.LAYERS, tc.BATCH, tc.C_COND, tc.HIDDEN, tc.SEED]))
  # the key set, learnt from the reference, bare and inside MeshTransformer
  n, s, r = tc.CASES["rand_k3"][0]()
  x, cond = tc.inputs("rand_k3", n)
  x64, c64 = x.astype(np.float64), cond.astype(np.float64)
  keys = _learn_keys(n, s, r, x64, c64, wrapped=False)
  assert keys == tc.param_specs(), sorted(set(keys) ^ set(tc.param_specs()))
  keys_mt = _learn_keys(n, s, r, np.transpose(x64, (1, 0, 2)), c64, wrapped=True)
  assert keys_mt == tc.param_specs(prefix="mesh_transformer/~/transformer/"), sorted(keys_mt)
  out["param_keys"] = np.array(sorted(keys))
  out["param_keys_mesh_transformer"] = np.array(sorted(keys_mt))
  params = {m: {leaf: v.astype(np.float64) for leaf, v in lv.items()}
            for m, lv in tc.init_params(tc.param_specs()).items()}
  out["params_sha256"] = np.array(oparams.digest(params))
  for case, (graph, k) in tc.CASES.items():
    n, s, r = graph()
    x, cond = tc.inputs(case, n)
    x64, c64 = x.astype(np.float64), cond.astype(np.float64)
    y = _run(n, s, r, k, "mha", x64, c64, params)
    y_tri = _run(n, s, r, k, "triblockdiag_mha", x64, c64, params)
    err = np.abs(y_tri - y).max() / np.abs(y).max()
    assert err < 1e-12, (case, err)
    mask = _adj(n, s, r) ** k
    mask.sort_indices()
    rows = tc.sample_rows(case, n)
    out[f"{case}_senders"], out[f"{case}_receivers"] = s.astype(np.int32), r.astype(np.int32)
    out[f"{case}_mask_indptr"] = mask.indptr.astype(np.int32)
    out[f"{case}_mask_indices"] = mask.indices.astype(np.int32)
    out[f"{case}_rows"] = rows
    out[f"{case}_y_f64"] = y[:, rows]
    out[f"{case}_tri_vs_mha"] = np.array(err)
    print(case, "n", n, "k", k, "mask nnz", mask.nnz, "tri vs mha", err)
  path = os.path.join(HERE, "transformer512.npz")
  np.savez_compressed(path, **out)
  print("wrote", path, os.path.getsize(path), "bytes")
  hpath = os.path.join(HERE, "banded_order_hashes.json")
  with open(hpath, "w") as f:
    json.dump(banded_hashes(), f, indent=1, sort_keys=True)
  print("wrote", hpath)


if __name__ == "__main__":
  main()
