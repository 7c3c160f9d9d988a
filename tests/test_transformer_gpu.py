"""GenCast's mesh transformer on the MI355X (graphcast_amd/sparse_transformer.py, csrc/attention.inc) against the
reference executed (tests/golden/transformer512.npz) and the fp64 oracle (tests/_transformer_oracle.py), in both
precisions."""
import os

import numpy as np
import pytest

from tests import _transformer_oracle as oracle
from tests.golden import transformer_case as tc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PRECS = ["f16x3", "f32"]


def _torch():
  import torch
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  return torch


@pytest.fixture(scope="module")
def golden():
  return np.load(os.path.join(HERE, "golden", "transformer512.npz"))


@pytest.fixture(scope="module")
def params():
  return tc.init_params(tc.param_specs())


def _model(n, s, r, k, params, prec, layers=tc.LAYERS, **kw):
  from graphcast_amd import sparse_transformer as st
  adj = st.adjacency(n, s, r)
  return st.Transformer(adj, attention_k_hop=k, attention_type="mha", mask_type="full", num_heads=tc.HEADS,
                        num_layers=layers, d_model=tc.D, ffw_hidden=tc.HIDDEN, params=params, precision=prec, **kw)


def _rel(a, b):
  return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _run(model, x, cond):
  torch = _torch()
  y = model(torch.from_numpy(x).cuda(), torch.from_numpy(cond).cuda())
  torch.cuda.synchronize()
  return y.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_golden(golden, params, case, prec):
  graph, k = tc.CASES[case]
  n, s, r = graph()
  x, cond = tc.inputs(case, n)
  y = _run(_model(n, s, r, k, params, prec), x, cond)
  rows = golden[f"{case}_rows"]
  want = golden[f"{case}_y_f64"]
  for b in range(tc.BATCH):
    err = _rel(y[b, rows], want[b])
    assert err <= 2e-5, (case, prec, b, err)


@pytest.mark.parametrize("prec", PRECS)
def test_m4_k16_16_layers_rows(params, prec):
  """M4, k = 16, 16 layers, batch 2 against the committed fp64-oracle row sample (scripts/make_transformer_rows.py)."""
  from graphcast_amd import icosahedral_mesh as im
  ref = np.load(os.path.join(HERE, "golden", "transformer_m4k16_rows.npz"))
  mesh = im.get_last_triangular_mesh_for_sphere(4)
  s, r = im.faces_to_edges(mesh.faces)
  n = mesh.vertices.shape[0]
  p16 = tc.init_params(tc.param_specs(num_layers=16), seed=int(ref["seed"]))
  rng = np.random.default_rng(int(ref["seed"]))
  x = rng.standard_normal((2, n, tc.D)).astype(np.float32)
  cond = rng.standard_normal((2, tc.C_COND)).astype(np.float32)
  y = _run(_model(n, s, r, 16, p16, prec, layers=16), x, cond)
  rows = ref["rows"]
  for b in range(2):
    err = _rel(y[b, rows], ref["y"][b])
    assert err <= 1e-5, (prec, b, err)


@pytest.fixture(scope="module")
def m6():
  from graphcast_amd import icosahedral_mesh as im
  mesh = im.get_last_triangular_mesh_for_sphere(6)
  s, r = im.faces_to_edges(mesh.faces)
  return mesh.vertices.shape[0], s, r, mesh.vertices


@pytest.mark.parametrize("prec", PRECS)
def test_m6_k16_one_layer_vs_oracle(params, m6, prec):
  from graphcast_amd import sparse_transformer as st
  n, s, r, pos = m6
  p1 = tc.init_params(tc.param_specs(num_layers=1), seed=3)
  rng = np.random.default_rng(3)
  x = rng.standard_normal((1, n, tc.D)).astype(np.float32)
  cond = rng.standard_normal((1, tc.C_COND)).astype(np.float32)
  model = _model(n, s, r, 16, p1, prec, layers=1, node_positions=pos)
  y = _run(model, x, cond)
  rows = np.sort(rng.choice(n, 512, replace=False))
  want = oracle.forward(p1, model.mask, x, cond, 1, rows=rows)
  err = _rel(y[:, rows], want)
  assert err <= 5e-6, (prec, err)


def test_m6_k16_16_layers_f16x3_vs_f32(m6):
  n, s, r, pos = m6
  p16 = tc.init_params(tc.param_specs(num_layers=16), seed=4)
  rng = np.random.default_rng(4)
  x = rng.standard_normal((1, n, tc.D)).astype(np.float32)
  cond = rng.standard_normal((1, tc.C_COND)).astype(np.float32)
  a = _run(_model(n, s, r, 16, p16, "f16x3", layers=16, node_positions=pos), x, cond)
  b = _run(_model(n, s, r, 16, p16, "f32", layers=16, node_positions=pos), x, cond)
  err = _rel(a, b)
  assert err <= 5e-6, err


@pytest.mark.parametrize("prec", PRECS)
def test_swapping_conditioning_rows_swaps_outputs(params, prec):
  n, s, r = tc.random_edges()
  x, cond = tc.inputs("rand_k3", n)
  x = np.stack([x[0], x[0]])                 # the same nodes, two different conditionings
  m = _model(n, s, r, 3, params, prec)
  y = _run(m, x, cond)
  y_sw = _run(m, x, cond[::-1].copy())
  assert not np.array_equal(y[0], y[1])
  assert np.array_equal(y_sw[0], y[1]) and np.array_equal(y_sw[1], y[0])


@pytest.mark.parametrize("prec", PRECS)
def test_isolated_node_ragged_size_and_large_logits(params, prec):
  """Node 41 of the random graph has no edge: its only key is itself (its attention output is its own v).  100 nodes
  is not a multiple of the 64-row tile.  q = k = v = 30 N(0, 1) puts logits near 1e4: no overflow."""
  from graphcast_amd import sparse_transformer as st
  n, s, r = tc.random_edges()
  x, cond = tc.inputs("rand_k3", n)
  model = _model(n, s, r, 3, params, prec)
  assert model.mask[41].indices.tolist() == [41] and n % 64 != 0
  y = _run(model, x, cond)
  want = oracle.forward(params, model.mask, x, cond, tc.LAYERS, rows=np.array([41, 0, 99]))
  assert _rel(y[:, [41, 0, 99]], want) <= 2e-5
  # large logits: the attention kernel alone on q, k, v = 30 N(0, 1) rows
  torch = _torch()
  rng = np.random.default_rng(9)
  qkv = [torch.from_numpy((30 * rng.standard_normal((1 * n, tc.D))).astype(np.float32)).cuda() for _ in range(3)]
  out = torch.empty_like(qkv[0])
  model.attention(*qkv, out, 1)
  torch.cuda.synchronize()
  model.check_range()
  order = model.tiles.order
  q, k, v = (t.cpu().numpy().astype(np.float64)[None] for t in qkv)
  perm_mask = model.mask[order][:, order]
  want = oracle.attention(q, k, v, perm_mask.tocsr())
  got = out.cpu().numpy()[None]
  assert np.isfinite(got).all()
  assert _rel(got, want) <= 2e-5, _rel(got, want)


@pytest.mark.parametrize("prec", PRECS)
def test_twenty_runs_bitwise_identical(params, prec):
  n, s, r = tc.m2_edges()
  x, cond = tc.inputs("m2_k4", n)
  m = _model(n, s, r, 4, params, prec)
  first = _run(m, x, cond)
  for _ in range(19):
    assert np.array_equal(_run(m, x, cond), first)


def test_f16x3_range_flag_raises_on_out_of_range_projections(params):
  from graphcast_amd import _native as nat
  n, s, r = tc.random_edges()
  x, cond = tc.inputs("rand_k3", n)
  m = _model(n, s, r, 3, params, "f16x3")
  torch = _torch()
  qkv = [torch.zeros((n, tc.D), dtype=torch.float32, device="cuda") for _ in range(3)]
  qkv[1][5, 7] = 1e6             # one K value beyond GC_F16X3_MAX
  out = torch.empty_like(qkv[0])
  m.attention(*qkv, out, 1)
  with pytest.raises(nat.GcastRangeError):
    m.check_range()
  m.check_range()                # (the flag was cleared by the raise)
  # end to end: a conditioning scale of 1e5 makes the projections' inputs out of range
  p = {k: dict(v) for k, v in params.items()}
  key = "transformer/block_00/block_00_norm_conditioning/linear"
  p[key]["b"] = p[key]["b"].copy()
  p[key]["b"][:tc.D] = 1e5
  m2 = _model(n, s, r, 3, p, "f16x3")
  with pytest.raises(nat.GcastRangeError):
    _run(m2, x, cond)


@pytest.mark.parametrize("prec", PRECS)
def test_mesh_transformer_round_trip(params, prec):
  torch = _torch()
  from graphcast_amd import transformer as gt
  from graphcast_amd import typed_graph
  case = "m2_k2"
  n, s, r = tc.m2_edges()
  x, cond = tc.inputs(case, n)
  p = {("mesh_transformer/~/" + k): v for k, v in params.items()}
  graph = typed_graph.TypedGraph(
      context=typed_graph.Context(n_graph=np.array([1]), features=()),
      nodes={"mesh_nodes": typed_graph.NodeSet(n_node=np.array([n]),
                                               features=torch.from_numpy(np.transpose(x, (1, 0, 2)).copy()).cuda())},
      edges={typed_graph.EdgeSetKey("mesh", ("mesh_nodes", "mesh_nodes")): typed_graph.EdgeSet(
          n_edge=np.array([len(s)]), indices=typed_graph.EdgesIndices(senders=s, receivers=r), features=())})
  mt = gt.MeshTransformer(None, dict(attention_k_hop=2, attention_type="triblockdiag_mha", mask_type="full",
                                     num_heads=4, num_layers=tc.LAYERS, d_model=tc.D, ffw_hidden=tc.HIDDEN),
                          name="mesh_transformer", params=p, precision=prec)
  out = mt(graph, torch.from_numpy(cond).cuda())
  y = out.nodes["mesh_nodes"].features
  assert tuple(y.shape) == (n, tc.BATCH, tc.D)
  g = np.load(os.path.join(HERE, "golden", "transformer512.npz"))
  rows = g[f"{case}_rows"]
  got = y.cpu().numpy().astype(np.float64).transpose(1, 0, 2)[:, rows]
  assert _rel(got, g[f"{case}_y_f64"]) <= 2e-5
