"""The alpha stage alone at 8192 x 8192 on the planes of measure.sh, run from the repository root (under rocprofv3, or plain):
    python profiles/alpha_early_out/alpha_planes.py <reps> <plane> [<plane> ...]
  a  the bench frame's alpha plane (yaik_amd/synth.py, seed 12345): 52.8 % of the tiles kept, every kept tile opaque in every row
  b  all 255: every tile decided by the probe
  c  all 0: every row of every tile read, nothing kept
  d  every tile kept by a single sample in row 14, a row the probe does not read: every byte read, in two dependent rounds
Per plane: REPS + 3 launches of yk_alpha_kernel (two to warm up, the REPS timed ones, one of the closing mip_prefilter); summarize.py
splits a trace by that count."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import torch
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

W = 8192
reps = int(sys.argv[1])
e = HipTileEncoder(0)
for name in sys.argv[2:]:
    if name == "a":
        planes = synth_planes_torch(W, n_planes=4, seed=12345, device="cuda")
    else:
        planes = torch.zeros((4, W, W), dtype=torch.int32, device="cuda")
        if name == "b":
            planes[3] = 255
        elif name == "d":
            planes[3].view(W // 16, 16, W // 16, 16)[:, 14, :, 7] = 1
    torch.cuda.synchronize()
    e.set_image(planes)
    for _ in range(reps + 2):
        e.alpha_reject()
        e.synchronize()
    r = e.mip_prefilter()
    print(f"plane {name}: bounds {r['bounds'].tolist()} kept tiles {r['remaining'] // 256 if r['has_chunk'] else (W // 16) ** 2} of {(W // 16) ** 2}", flush=True)
    del planes
e.close()
