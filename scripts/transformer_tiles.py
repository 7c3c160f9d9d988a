#!/usr/bin/env python
"""Structure of the k-hop attention mask in 64 x 64 tiles (host only, no GPU): for GenCast's meshes M4 / M5 / M6
(finest level only) at attention_k_hop 16, the key tiles each query tile touches and the mask density inside them,
for the reference's reverse Cuthill-McKee order (icosahedral_mesh.get_permutation_to_banded) and for the 3-D Morton
order of the vertices.  One JSON line per (mesh, order).

    python scripts/transformer_tiles.py [--levels 4 5 6] [--k 16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--levels", type=int, nargs="+", default=[4, 5, 6])
  ap.add_argument("--k", type=int, default=16)
  a = ap.parse_args()
  from graphcast_amd import icosahedral_mesh as im
  from graphcast_amd import sparse_transformer as st
  for level in a.levels:
    mesh = im.get_last_triangular_mesh_for_sphere(level)
    s, r = im.faces_to_edges(mesh.faces)
    n = mesh.vertices.shape[0]
    t0 = time.perf_counter()
    mask = st.k_hop_mask(st.adjacency(n, s, r), a.k)
    mask_s = time.perf_counter() - t0
    for name, order in (("rcm_banded", im.get_permutation_to_banded(mesh)[0]),
                        ("morton3d", st.morton_order(mesh.vertices))):
      t = st.Tiles(mask, order)
      print(json.dumps(dict(mesh=f"M{level}", nodes=n, k_hop=a.k, order=name, mask_nnz=int(mask.nnz),
                            **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in t.stats().items()},
                            mask_seconds=round(mask_s, 1))), flush=True)


if __name__ == "__main__":
  main()
