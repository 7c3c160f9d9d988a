"""GPU, BASELINE.json configs[2] ITSELF: the 10-day autoregressive rollout -- 40 x 6-h steps -- at 0.25 deg / 37 levels /
M6 (16 processor steps) on one MI355X: rollout_device.DeviceRollout (the step + gc_advance_state, state resident in
HBM) against the oracle through the reference's own demo stack, rollout.chunked_prediction (utils/rollout.py:326-565)
around normalization.InputsAndResiduals (utils/normalization.py:113-160) around a Predictor whose step is the fp32
torch-CPU restatement.

The oracle side is a committed fixture, tests/golden/rollout40_0p25deg_rows.npz: 256 sampled grid rows x 227 channels
per lead time, generated in the build container by `python tests/golden/make_golden_rollout40.py --config 0p25deg40`
(40 full oracle steps, ~115 s each on 8 cores; the generator rewrites the file after every step, the test takes the
number of lead times from it).  Seeded inputs / statistics / parameters are regenerated here and their digest
checked.  Tolerances as in tests/test_rollout40_gpu.py (the 1 deg run): rel-RMSE over all predicted variables
<= 2e-5 at step 1, <= 1e-4 (BASELINE.json's budget) at every later step."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from graphcast_amd import graphcast as gc          # noqa: E402
from graphcast_amd import rollout_device           # noqa: E402
from tests.golden import make_golden_rollout40 as G   # noqa: E402

FIXTURE = "rollout40_0p25deg_rows.npz"


@pytest.mark.gpu
def test_forty_step_rollout_at_headline_size(golden_dir):
  if not torch.cuda.is_available():
    pytest.fail("GPU test selected but no GPU is visible")
  cfg = G.CONFIGS["0p25deg40"]
  z = np.load(os.path.join(golden_dir, FIXTURE))
  want = z["traj"].astype(np.float64)
  n_have = want.shape[0]
  assert n_have == cfg.n_steps, f"the committed oracle trajectory holds {n_have} of {cfg.n_steps} lead times"
  params, inputs, template, forcings, (mean, std, dstd), _ = G.setup("0p25deg40")
  assert G.digest(params, inputs, forcings) == str(z["inputs_sha256"])
  mc = gc.ModelConfig(resolution=cfg.res, mesh_size=cfg.mesh, latent_size=512, gnn_msg_steps=G.GNN_STEPS,
                      hidden_layers=1, radius_query_fraction_edge_length=0.6)
  model = gc.GraphCast(mc, cfg.task, params=params).init_from_coordinates(cfg.lat, cfg.lon)
  rows = G.fixture_rows(z, "0p25deg40", model.graph_arrays())            # (the sampling rule re-applied to the PRODUCT's graph)
  roll = rollout_device.DeviceRollout(model, std, mean, dstd)
  traj = roll.run(inputs, template, forcings)                      # [40, N_grid, 1, C_out], de-normalised: 38 GB in HBM
  torch.cuda.synchronize()
  assert torch.isfinite(traj).all()
  got = traj[:, torch.as_tensor(rows, device=traj.device), 0].cpu().numpy().astype(np.float64)
  per_step = [float(np.linalg.norm(got[s] - want[s]) / np.linalg.norm(want[s])) for s in range(n_have)]
  report = {"config": "0.25deg_37L_M6, 16 processor steps, 40 autoregressive steps, 256 sampled grid rows x 227 channels",
            "oracle": f"tests/golden/{FIXTURE} (torch-CPU fp32 oracle through rollout.chunked_prediction + InputsAndResiduals)",
            "rel_rmse_step_1_10_20_30_40": [per_step[k] for k in (0, 9, 19, 29, 39)], "rel_rmse_max": max(per_step),
            "rel_rmse_per_step": per_step}       # (timing of this loop: `rollout` of bench.py --full -- here the first step builds the engine)
  print("ROLLOUT40_FULLSIZE_PARITY " + json.dumps(report))
  out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
  os.makedirs(out_dir, exist_ok=True)
  with open(os.path.join(out_dir, "rollout40_fullsize_parity.json"), "w") as f:
    json.dump(report, f, indent=1)
  assert per_step[0] <= 2e-5
  assert max(per_step) <= 1e-4
