#!/usr/bin/env python
"""Times GenCast's mesh transformer on the device (graphcast_amd/sparse_transformer.py): M4 / M5 / M6 (finest level
only), attention_k_hop 16, 16 layers, batch 1, both precisions.  One JSON line per case: ms per call, ms per attention
launch, the tiles the mask touches, and the useful (mask entries) vs tile-level attention FLOPs with the fraction of
the 2.5 PF/s f16 MFMA peak the call reaches on all its FLOPs (dense layers + tile-level attention).

    python scripts/transformer_bench.py [--levels 4 5 6] [--iters 5] [--order morton|rcm]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 2.5e15


def params(layers, c_cond=16, seed=0):
  rng = np.random.default_rng(seed)
  d, h = 512, 2048
  out = {}
  lin = lambda k, n: {"w": (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32),
                      "b": (0.1 * rng.standard_normal(n)).astype(np.float32)}
  cnd = lambda: {"w": (0.3 / np.sqrt(c_cond) * rng.standard_normal((c_cond, 2 * d))).astype(np.float32),
                 "b": (0.1 * rng.standard_normal(2 * d)).astype(np.float32)}
  for i in range(layers):
    blk = f"transformer/block_{i:02d}/"
    for p in "qkv":
      out[blk + f"mha_proj_{p}"] = {"w": lin(d, d)["w"]}
    out[blk + "mha_final"] = lin(d, d)
    out[blk + "ffw_up"] = lin(d, h)
    out[blk + "ffw_down"] = lin(h, d)
    out[blk + f"block_{i:02d}_norm_conditioning/linear"] = cnd()
    out[blk + f"block_{i:02d}_norm_conditioning_1/linear"] = cnd()
  out["transformer/transformer_final_norm_conditioning/linear"] = cnd()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--levels", type=int, nargs="+", default=[4, 5, 6])
  ap.add_argument("--precisions", nargs="+", default=["f16x3", "f32"])
  ap.add_argument("--layers", type=int, default=16)
  ap.add_argument("--k", type=int, default=16)
  ap.add_argument("--iters", type=int, default=5)
  ap.add_argument("--order", choices=["morton", "rcm"], default="morton")
  a = ap.parse_args()
  import torch
  from graphcast_amd import icosahedral_mesh as im
  from graphcast_amd import sparse_transformer as st
  p = params(a.layers)
  for level in a.levels:
    mesh = im.get_last_triangular_mesh_for_sphere(level)
    s, r = im.faces_to_edges(mesh.faces)
    n = mesh.vertices.shape[0]
    t0 = time.perf_counter()
    pos = mesh.vertices if a.order == "morton" else None
    mask, tiles = st.tiles_for(n, s, r, a.k, positions=pos)
    host_s = time.perf_counter() - t0
    rng = np.random.default_rng(level)
    x = torch.from_numpy(rng.standard_normal((1, n, 512)).astype(np.float32)).cuda()
    cond = torch.from_numpy(rng.standard_normal((1, 16)).astype(np.float32)).cuda()
    for prec in a.precisions:
      model = st.Transformer(st.adjacency(n, s, r), attention_k_hop=a.k, attention_type="splash_mha", num_heads=4,
                             num_layers=a.layers, d_model=512, ffw_hidden=2048, params=p, precision=prec,
                             node_positions=pos)
      model(x, cond)
      torch.cuda.synchronize()
      ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
      ev[0].record()
      for _ in range(a.iters):
        model(x, cond, check_range=False)
      ev[1].record()
      torch.cuda.synchronize()
      model.check_range()
      ms_call = ev[0].elapsed_time(ev[1]) / a.iters
      b = model._buffers(1)
      ev[0].record()
      for _ in range(a.iters * 4):
        model.attention(b["q"], b["k"], b["v"], b["att"], 1)
      ev[1].record()
      torch.cuda.synchronize()
      ms_att = ev[0].elapsed_time(ev[1]) / (a.iters * 4)
      dense = a.layers * n * 2 * 512 * (4 * 512 + 2 * 2048)
      useful = a.layers * 4 * mask.nnz * 2 * 2 * 128
      tile_level = a.layers * 4 * tiles.n_tiles * 64 * 64 * 2 * 2 * 128
      st_ = tiles.stats()
      print(json.dumps(dict(
          mesh=f"M{level}", nodes=n, k_hop=a.k, layers=a.layers, batch=1, precision=prec, order=a.order,
          ms_per_call=round(ms_call, 3), ms_per_attention=round(ms_att, 4),
          query_tiles=st_["query_tiles"], tiles=st_["tiles"], tiles_per_query_tile=round(st_["tiles_per_query_tile"], 2),
          mask_density_in_tiles=round(st_["density"], 4), dense_gflop=round(dense / 1e9, 1),
          attention_useful_gflop=round(useful / 1e9, 1), attention_tile_gflop=round(tile_level / 1e9, 1),
          fraction_of_2p5PF=round((dense + tile_level) / (ms_call * 1e-3) / PEAK, 4),
          host_mask_and_tiles_s=round(host_s, 2))), flush=True)
      del model
      torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
