"""Drop-in for the helpers of ``lie_vae.experiments.utils`` the package uses (reference
lie_vae/experiments/utils.py): the schedules live in train_dp and are re-exported here."""
from .train_dp import ConstantSchedule, LinearSchedule  # noqa: F401


def expand_dim(x, n, dim=0):
    """Insert an axis of size n at ``dim`` as a stride-0 expand (experiments/utils.py:82-85)."""
    if dim < 0:
        dim = x.dim() + dim + 1
    return x.unsqueeze(dim).expand(*[-1] * dim, n, *[-1] * (x.dim() - dim))
