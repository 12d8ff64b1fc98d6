"""Generate tests/golden/so3_log.npz by running the REFERENCE's own rodrigues and log_map on
the CPU (build container only, like oracle/gen_golden.py, whose reference path and stub
packages this script reuses).

Run:  python tools/gen_so3_log_golden.py

256 seeded rotations, axes uniform on the sphere and theta uniform in [0.05, pi - 0.05] (the
range in which the reference's acos / sin expression keeps its digits in fp64).  R comes from
the reference's rodrigues in fp64; its log_map, which is unbatched, is applied one matrix at a
time in fp64 (v64) and again on R.float() (v32_ref, the reference's own fp32 answer).  The
file holds data only: R, v64, v32_ref.
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import _install_stubs, _np  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "so3_log.npz")
N = 256


def main():
    _install_stubs()
    from lie_vae import lie_tools as lt

    g = torch.Generator().manual_seed(3107)
    axis = torch.randn(N, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    theta = 0.05 + torch.rand(N, generator=g, dtype=torch.float64) * (math.pi - 0.1)
    R = lt.rodrigues(axis * theta[:, None])
    v64 = torch.stack([lt.map_to_lie_vector(lt.log_map(r)) for r in R])
    v32 = torch.stack([lt.map_to_lie_vector(lt.log_map(r)) for r in R.float()])
    assert v64.dtype == torch.float64 and v32.dtype == torch.float32
    assert (v64 - axis * theta[:, None]).abs().max() < 1e-12
    np.savez(OUT, R=_np(R), v64=_np(v64), v32_ref=_np(v32))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 64 * 1024


if __name__ == "__main__":
    main()
