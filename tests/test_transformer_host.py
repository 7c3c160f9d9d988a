"""Host side of GenCast's mesh transformer (graphcast_amd/sparse_transformer.py): the fp64 oracle against the reference
executed (tests/golden/transformer512.npz), the k-hop mask and its tiles, the banded mesh order, the API's refusals,
and the attention kernels' build (cross-compiled: no GPU needed)."""
import json
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import _transformer_oracle as oracle
from tests.golden import transformer_case as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden():
  return np.load(os.path.join(GOLDEN, "transformer512.npz"))


def test_seeded_parameters_are_the_reference_tree(golden):
  from oracle import params as oparams
  assert sorted(golden["param_keys"].tolist()) == sorted(tc.param_specs())
  assert sorted(golden["param_keys_mesh_transformer"].tolist()) == sorted(
      tc.param_specs(prefix="mesh_transformer/~/transformer/"))
  p = {m: {leaf: v.astype(np.float64) for leaf, v in lv.items()} for m, lv in tc.init_params(tc.param_specs()).items()}
  assert oparams.digest(p) == str(golden["params_sha256"])


@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_oracle_matches_reference(golden, case):
  graph, k = tc.CASES[case]
  n, s, r = graph()
  x, cond = tc.inputs(case, n)
  mask = oracle.k_hop_mask(n, s, r, k)
  y = oracle.forward(tc.init_params(tc.param_specs()), mask, x, cond, tc.LAYERS, rows=golden[f"{case}_rows"])
  want = golden[f"{case}_y_f64"]
  assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
  assert float(golden[f"{case}_tri_vs_mha"]) < 1e-12     # triblockdiag_mha == mha in the reference itself


@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_host_mask_is_the_reference_mask(golden, case):
  from graphcast_amd import sparse_transformer as st
  graph, k = tc.CASES[case]
  n, s, r = graph()
  assert np.array_equal(np.asarray(golden[f"{case}_senders"]), s)
  mask = st.k_hop_mask(st.adjacency(n, s, r), k)
  want = np.zeros((n, n), bool)
  ip, ix = golden[f"{case}_mask_indptr"], golden[f"{case}_mask_indices"]
  want[np.repeat(np.arange(n), np.diff(ip)), ix] = True
  assert np.array_equal(mask.toarray(), want)


def _check_tiles(mask, tiles):
  n = mask.shape[0]
  dense = np.zeros((n, n), np.int64)
  inv = tiles.inverse
  nq = tiles.n_qtiles
  assert len(tiles.ptr) == nq + 1 and tiles.ptr[-1] == tiles.n_tiles
  for qt in range(nq):
    cols = tiles.col[tiles.ptr[qt]:tiles.ptr[qt + 1]]
    assert (np.diff(cols) > 0).all()
    for t in range(tiles.ptr[qt], tiles.ptr[qt + 1]):
      words = tiles.bits[t * 64:(t + 1) * 64]
      assert words.any()
      for rr in range(64):
        w = int(words[rr])
        i = qt * 64 + rr
        if w:
          assert i < n
        for c in range(64):
          if (w >> c) & 1:
            j = tiles.col[t] * 64 + c
            assert j < n
            dense[i, j] += 1
  # every mask entry covered by exactly one bit, and no bit outside the mask
  want = mask.toarray()[tiles.order][:, tiles.order].astype(np.int64)
  assert np.array_equal(dense, want)
  assert np.array_equal(tiles.order[inv], np.arange(n))


@pytest.mark.parametrize("case", sorted(tc.CASES))
def test_tiles_cover_the_mask_exactly(case):
  from graphcast_amd import sparse_transformer as st
  graph, k = tc.CASES[case]
  n, s, r = graph()
  mask, tiles = st.tiles_for(n, s, r, k)
  _check_tiles(mask, tiles)
  assert st.tiles_for(n, s, r, k)[1] is tiles            # cached on the index bytes


def test_tiles_cover_the_mask_in_morton_order():
  from graphcast_amd import icosahedral_mesh as im
  from graphcast_amd import sparse_transformer as st
  mesh = im.get_last_triangular_mesh_for_sphere(3)
  s, r = im.faces_to_edges(mesh.faces)
  mask, tiles = st.tiles_for(mesh.vertices.shape[0], s, r, 3, positions=mesh.vertices)
  assert sorted(tiles.order.tolist()) == list(range(mesh.vertices.shape[0]))
  _check_tiles(mask, tiles)


@pytest.mark.parametrize("level", [4, 5, 6])
def test_banded_permutation_matches_reference(level):
  from graphcast_amd import icosahedral_mesh as im
  want = json.load(open(os.path.join(GOLDEN, "banded_order_hashes.json")))[f"M{level}"]
  perm, func = im.get_permutation_to_banded(im.get_last_triangular_mesh_for_sphere(level))
  assert len(perm) == want["n"]
  assert hashlib.sha256(np.asarray(perm, np.int64).tobytes()).hexdigest() == want["sha256"]
  assert np.array_equal(func(perm), np.arange(len(perm)))


def test_unsupported_shapes_raise():
  from graphcast_amd import sparse_transformer as st
  n, s, r = tc.random_edges()
  adj = st.adjacency(n, s, r)
  base = dict(attention_k_hop=2, attention_type="mha", mask_type="full", num_heads=4, num_layers=1, d_model=512,
              ffw_hidden=2048, params={})
  for bad in (dict(d_model=256), dict(key_size=64, num_heads=8), dict(ffw_hidden=1024), dict(activation="relu"),
              dict(dtype="bfloat16")):
    with pytest.raises(NotImplementedError):
      st.Transformer(adj, **{**base, **bad})
  with pytest.raises(ValueError):
    st.Transformer(adj, **{**base, "attention_type": "dense"})


def test_spatial_norm_conditioning_is_refused():
  from graphcast_amd import sparse_transformer as st
  with pytest.raises(NotImplementedError):
    st.check_global_conditioning(np.zeros((2, 10, 16), np.float32))


def test_attention_kernels_cross_compile_and_are_hazard_free(tmp_path):
  if shutil.which("hipcc") is None:
    pytest.skip("hipcc not on PATH")
  out = str(tmp_path / "gcast.s")
  cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-inline-asm", "-S",
         "--cuda-device-only", "-DGC_PIPE=2", '-DGC_SRC_HASH="x"', "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "graphcast_amd", "csrc", "gcast.hip"), "-o", out]
  subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
  sys.path.insert(0, os.path.join(ROOT, "scripts"))
  import asm_hazard_check as chk
  names = ("attn_tile_kernel", "ln_cond_kernel", "gelu_kernel", "permute_rows_kernel")
  kernels = {name: lines for name, lines in chk.functions(out).items() if any(k in name for k in names)}
  assert sum("attn_tile_kernel" in k for k in kernels) == 2 and len(kernels) == 5
  bad = {name: chk.check(lines)[:4] for name, lines in kernels.items()}
  assert not {k: v for k, v in bad.items() if v}
