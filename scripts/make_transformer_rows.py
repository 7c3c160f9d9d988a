#!/usr/bin/env python
"""Writes tests/golden/transformer_m4k16_rows.npz: the fp64 oracle (tests/_transformer_oracle.py) of GenCast's mesh
transformer at its published depth and reach -- 16 layers, attention_k_hop 16 -- on the M4 mesh (2,562 nodes, finest
level only), batch 2, seeded parameters and inputs, at 64 sampled rows.  The oracle itself is pinned to the reference
executed by tests/test_transformer_host.py.

    python scripts/make_transformer_rows.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graphcast_amd import icosahedral_mesh as im          # noqa: E402
from tests import _transformer_oracle as oracle           # noqa: E402
from tests.golden import transformer_case as tc           # noqa: E402

SEED = 16


def main():
  mesh = im.get_last_triangular_mesh_for_sphere(4)
  s, r = im.faces_to_edges(mesh.faces)
  n = mesh.vertices.shape[0]
  params = tc.init_params(tc.param_specs(num_layers=16), seed=SEED)
  rng = np.random.default_rng(SEED)
  x = rng.standard_normal((2, n, tc.D)).astype(np.float32)
  cond = rng.standard_normal((2, tc.C_COND)).astype(np.float32)
  rows = np.sort(np.random.default_rng(SEED + 1).choice(n, 64, replace=False))
  mask = oracle.k_hop_mask(n, s, r, 16)
  y = oracle.forward(params, mask, x, cond, 16, rows=rows)
  path = os.path.join(ROOT, "tests", "golden", "transformer_m4k16_rows.npz")
  np.savez_compressed(path, seed=np.array(SEED), rows=rows, y=y, mask_nnz=np.array(mask.nnz))
  print("wrote", path, os.path.getsize(path), "bytes; mask nnz", mask.nnz)


if __name__ == "__main__":
  main()
