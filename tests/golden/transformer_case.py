"""The seeded cases of tests/golden/transformer512.npz -- graphs, sizes, parameters, inputs, sampled rows -- in a module
WITHOUT reference imports: the generator (make_golden_transformer.py, on a host with the reference sources) and the
tests (CPU and GPU hosts) both take them from here."""
import numpy as np

D, HEADS, LAYERS, BATCH, C_COND, HIDDEN = 512, 4, 2, 2, 16, 2048
SEED = 23
ROWS_PER_CASE = 16          # fp64 output rows stored per case (the fixture stays below 1 MiB)


def m2_edges():
  """GenCast's mesh edge set at refinement 2 (finest level only, 162 nodes): faces_to_edges of the last mesh."""
  from graphcast_amd import icosahedral_mesh as im
  mesh = im.get_last_triangular_mesh_for_sphere(2)
  s, r = im.faces_to_edges(mesh.faces)
  return mesh.vertices.shape[0], s.astype(np.int64), r.astype(np.int64)


def random_edges():
  """A small NON-symmetric random graph (100 nodes) with one isolated node (41: no edge in or out, so its only
  allowed key is itself) and a node without out-edges."""
  rng = np.random.default_rng(7)
  n = 100
  s = rng.integers(0, n, 260)
  r = rng.integers(0, n, 260)
  keep = (s != 41) & (r != 41) & (s != 77)
  return n, s[keep].astype(np.int64), r[keep].astype(np.int64)


# name -> (graph builder, attention_k_hop)
CASES = {"m2_k2": (m2_edges, 2), "m2_k4": (m2_edges, 4), "rand_k3": (random_edges, 3)}
ISOLATED = {"rand_k3": 41}


def param_specs(num_layers=LAYERS, prefix="transformer/", name="transformer", c_cond=C_COND):
  """{module: {leaf: shape}} of sparse_transformer.Transformer (as executing the reference reports it; the generator
  asserts the equality)."""
  specs = {}
  for i in range(num_layers):
    blk = f"{prefix}block_{i:02d}/"
    for p in "qkv":
      specs[blk + f"mha_proj_{p}"] = {"w": (D, D)}
    specs[blk + "mha_final"] = {"w": (D, D), "b": (D,)}
    specs[blk + "ffw_up"] = {"w": (D, HIDDEN), "b": (HIDDEN,)}
    specs[blk + "ffw_down"] = {"w": (HIDDEN, D), "b": (D,)}
    for sfx in ("", "_1"):
      specs[blk + f"block_{i:02d}_norm_conditioning{sfx}/linear"] = {"w": (c_cond, 2 * D), "b": (2 * D,)}
  specs[f"{prefix}{name}_final_norm_conditioning/linear"] = {"w": (c_cond, 2 * D), "b": (2 * D,)}
  return specs


def init_params(specs, seed=SEED):
  """Non-trivial seeded parameters (float32 values): Linear w ~ N(0, 1 / fan_in), biases ~ N(0, 0.1^2), conditioning
  w ~ N(0, 0.3^2 / C) -- so that every term of the block, the conditioning included, moves the output."""
  rng = np.random.default_rng(seed)
  out = {}
  for mod in sorted(specs):
    leafs = {}
    for leaf in sorted(specs[mod]):
      shape = specs[mod][leaf]
      if leaf == "b":
        a = 0.1 * rng.standard_normal(shape)
      elif "norm_conditioning" in mod:
        a = (0.3 / np.sqrt(shape[0])) * rng.standard_normal(shape)
      else:
        a = rng.standard_normal(shape) / np.sqrt(shape[0])
      leafs[leaf] = a.astype(np.float32)
    out[mod] = leafs
  return out


def inputs(case, n):
  """x [B, N, D] and global_norm_conditioning [B, C] (float32 values)."""
  rng = np.random.default_rng(1000 + sorted(CASES).index(case))
  x = rng.standard_normal((BATCH, n, D)).astype(np.float32)
  cond = rng.standard_normal((BATCH, C_COND)).astype(np.float32)
  return x, cond


def sample_rows(case, n):
  rng = np.random.default_rng(55 + sorted(CASES).index(case))
  rows = set(rng.choice(n, ROWS_PER_CASE, replace=False).tolist())
  if case in ISOLATED:
    rows.discard(sorted(rows)[0])
    rows.add(ISOLATED[case])
  return np.array(sorted(rows), dtype=np.int64)
