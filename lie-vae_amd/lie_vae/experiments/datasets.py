"""Datasets of the reference's lie_vae/experiments/datasets.py that the kernels can produce.

``ToyDataset`` (datasets.py:129-162): Haar-random poses q, one shared random spectrum scaled
to Frobenius norm 10, and targets
x = block_wigner_matrix_multiply(quaternions_to_eazyz(q), spectrum, degrees).

``SphereCubeDataset`` / ``ScPairsDataset`` (datasets.py:87-127): the reference reads PNGs that
Blender rendered from cube.blend; here the images come from the project's own sphere-cube
scene (csrc/render.hip), rendered on the device from the poses, with the
reference's item layout ``(name, group_el, image)``.  ``spherecube_batch`` renders a fresh
batch per training step.

``MeshDataset`` is the reference's ShapeDataset (datasets.py:18-85: many objects, a per-object
``name``, ``single_id = False``) with the images rendered on the device from triangle meshes
(csrc/render_mesh.hip) instead of read from directories of rendered ShapeNet
objects; ``mesh_batch`` renders a fresh batch per training step.

All maps run in liblievae_hip.so, so every ``generate`` needs a GPU device (the product path
has no CPU fallback).  Reading the reference's PNG directories and the ShapeNet reader stay
out of scope: MeshDataset takes its place for users who hold meshes.
"""
import math

import torch
from torch.utils.data import Dataset, TensorDataset

from ..lie_tools import (block_wigner_matrix_multiply, quaternions_to_eazyz, random_group_matrices,
                         random_quaternions, render_mesh, render_spherecube, rodrigues)
from ..meshes import MeshSet


def toy_harmonics(degrees=6, rep_copies=10, device=None):
    """Spectrum ((degrees+1)^2, rep_copies) with norm 10, drawn from the CURRENT RNG
    stream of ``device`` (datasets.py:146-147); the caller seeds (datasets.py:144-145)."""
    h = torch.randn((degrees + 1) ** 2, rep_copies, device=device)
    return h / h.norm() * 10


class ToyDataset(TensorDataset):
    """Tensors (q (n,4), harmonics (n,M,C) stride-0 expand, x (n,M,C))."""
    num_workers = 0
    single_id = True
    rgb = False

    def __init__(self, tensors=None, device=None, path='data/toy.pt'):
        if tensors is None:
            # The reference pickles with torch.save; here only tensor payloads are read
            # back (weights_only=True executes nothing from the file).
            tensors = torch.load(path, weights_only=True)
        if device is not None:
            tensors = [t.to(device) for t in tensors]
        super().__init__(*tensors)

    @classmethod
    def generate(cls, n=1000, degrees=6, rep_copies=10, device=None, batch_size=64,
                 harmonics=None):
        """datasets.py:143-158: seed 0, spectrum first, then one Haar batch of poses per
        ``batch_size`` chunk, each pushed through the fused ZYZ + Wigner-D action.
        ``harmonics`` (extension): a given ((degrees+1)^2, rep_copies) spectrum, e.g. of
        ``lie_vae.s2.project``, instead of the random draw; the poses then follow the seed
        directly."""
        # One seed, then spectrum and every pose batch from the same device stream, in the
        # reference's order (datasets.py:144-151): torch.manual_seed(0) seeds the CPU and
        # every CUDA generator, exactly like the reference's manual_seed + cuda.manual_seed.
        torch.manual_seed(0)
        if harmonics is None:
            harmonics = toy_harmonics(degrees, rep_copies, device)
        else:
            assert tuple(harmonics.shape) == ((degrees + 1) ** 2, rep_copies), \
                f"harmonics must be ({(degrees + 1) ** 2},{rep_copies}), got {tuple(harmonics.shape)}"
            harmonics = harmonics.detach().to(device=device, dtype=torch.float32)
        xs, qs = [], []
        for i in range(0, n, batch_size):
            batch_n = min(i + batch_size, n) - i
            q = random_quaternions(batch_n, device=device)
            x = block_wigner_matrix_multiply(
                quaternions_to_eazyz(q), harmonics.expand(batch_n, -1, -1), degrees)
            xs.append(x)
            qs.append(q)
        return cls(tensors=(torch.cat(qs, 0), harmonics.expand(n, -1, -1), torch.cat(xs, 0)),
                   device=device)

    def save(self, path='data/toy.pt'):
        q, h, x = self.tensors
        torch.save((q.cpu(), h.cpu().contiguous(), x.cpu()), path)


RENDER_CHUNK = 4096  # images in flight per render call while a dataset is generated


def _render_chunked(g, size, samples):
    """Images (n,3,size,size) of the poses g (n,3,3), at most RENDER_CHUNK per launch."""
    return torch.cat([render_spherecube(g[i:i + RENDER_CHUNK], size=size, samples=samples)
                      for i in range(0, max(g.shape[0], 1), RENDER_CHUNK)], 0)


def spherecube_batch(n, device, generator=None, size=64, samples=2):
    """A fresh batch for one training step: Haar poses g (n,3,3) and their images x
    (n,3,size,size), both on ``device``.  Two draws and two kernels on the current stream; no
    host read (``generator``: a torch.Generator of ``device``, default the device's stream)."""
    g = random_group_matrices(n, device=device, generator=generator)
    return g, render_spherecube(g, size=size, samples=samples)


class SphereCubeDataset(Dataset):
    """Items ``(0, group_el (3,3), image (3,size,size))`` as the reference's
    SphereCubeDataset (datasets.py:87-92 over ShapeDataset.load_file), backed by the tensors
    (g (n,3,3), x (n,3,size,size)) instead of a directory of PNGs."""
    num_workers = 0
    single_id = True
    rgb = True

    def __init__(self, tensors=None, device=None, path='data/spherecube.pt'):
        if tensors is None:
            tensors = torch.load(path, weights_only=True)
        if device is not None:
            tensors = [t.to(device) for t in tensors]
        self.tensors = tuple(tensors)
        g, x = self.tensors
        assert g.shape[0] == x.shape[0] and tuple(g.shape[-2:]) == (3, 3), \
            f"tensors must be (g (n,3,3), x (n,3,H,W)), got {tuple(g.shape)}, {tuple(x.shape)}"

    @classmethod
    def generate(cls, n=1000, size=64, device=None, generator=None, samples=2):
        """n Haar poses (random_group_matrices) and their renders."""
        g = random_group_matrices(n, device=device, generator=generator)
        return cls(tensors=(g, _render_chunked(g, size, samples)))

    def __len__(self):
        return self.tensors[0].shape[0]

    def __getitem__(self, idx):
        g, x = self.tensors
        return 0, g[idx], x[idx]

    def save(self, path='data/spherecube.pt'):
        torch.save(tuple(t.cpu() for t in self.tensors), path)

    @staticmethod
    def prep_batch(batch):
        return batch


class ScPairsDataset(SphereCubeDataset):
    """Items ``(names (2,), gs (2,3,3), imgs (2,3,size,size))`` of two nearby poses, as the
    reference's ScPairsDataset (datasets.py:95-127); tensors (g (num,2,3,3),
    x (num,2,3,size,size)).  ``prep_batch`` flattens the pairs of a collated batch."""

    def __init__(self, tensors=None, device=None, path='data/sc-pairs.pt'):
        super().__init__(tensors, device, path)

    @classmethod
    def generate(cls, num=1000, step_size=2 * math.pi / 60, size=64, device=None, generator=None,
                 samples=2):
        """gen_spherecube_pairs.py:10-14: a Haar, b = a·rodrigues(randn·step_size)."""
        a = random_group_matrices(num, device=device, generator=generator)
        step = torch.randn(num, 3, device=device, generator=generator) * step_size
        g = torch.stack([a, a.bmm(rodrigues(step))], 1)
        x = _render_chunked(g.reshape(-1, 3, 3), size, samples)
        return cls(tensors=(g, x.reshape(num, 2, *x.shape[1:])))

    def __getitem__(self, idx):
        g, x = self.tensors
        return torch.zeros(2, dtype=torch.long), g[idx], x[idx]

    def save(self, path='data/sc-pairs.pt'):
        super().save(path)

    @staticmethod
    def prep_batch(batch):
        return [t.view(-1, *t.shape[2:]) for t in batch]  # Flatten pairs


def _mesh_set(meshes, device):
    """``meshes`` as a MeshSet on ``device``: a MeshSet is taken as it is, a Mesh or a list of
    Mesh is packed (the one host sync of mesh rendering)."""
    return meshes if isinstance(meshes, MeshSet) else MeshSet(meshes, device)


def _render_mesh_chunked(g, meshes, names, size, samples):
    """Images (n,3,size,size) of mesh names[i] at pose g[i], at most RENDER_CHUNK per launch."""
    return torch.cat([render_mesh(g[i:i + RENDER_CHUNK], meshes, names[i:i + RENDER_CHUNK],
                                  size=size, samples=samples)
                      for i in range(0, max(g.shape[0], 1), RENDER_CHUNK)], 0)


def mesh_batch(n, device, meshes, generator=None, size=64, samples=2):
    """A fresh batch for one training step: a uniformly random mesh per item (names (n,)
    int64), Haar poses g (n,3,3) and the images x (n,3,size,size), all on ``device``.
    ``meshes``: a MeshSet (then no host read happens here), a Mesh or a list of Mesh."""
    meshes = _mesh_set(meshes, device)
    names = torch.randint(meshes.K, (n,), device=device, generator=generator)
    g = random_group_matrices(n, device=device, generator=generator)
    return names, g, render_mesh(g, meshes, names, size=size, samples=samples)


class MeshDataset(Dataset):
    """Items ``(name, group_el (3,3), image (3,size,size))`` as the reference's ShapeDataset
    (datasets.py:72-85), ``name`` the index of the item's mesh; backed by the tensors
    (names (n,) int64, g (n,3,3), x (n,3,size,size))."""
    num_workers = 0
    single_id = False
    rgb = True

    def __init__(self, tensors=None, device=None, path='data/meshes.pt'):
        if tensors is None:
            tensors = torch.load(path, weights_only=True)
        if device is not None:
            tensors = [t.to(device) for t in tensors]
        self.tensors = tuple(tensors)
        names, g, x = self.tensors
        assert names.dtype == torch.int64 and names.dim() == 1 and \
            names.shape[0] == g.shape[0] == x.shape[0] and tuple(g.shape[-2:]) == (3, 3), \
            "tensors must be (names (n,) int64, g (n,3,3), x (n,3,H,W)), got " \
            f"{tuple(names.shape)} {names.dtype}, {tuple(g.shape)}, {tuple(x.shape)}"

    @classmethod
    def generate(cls, meshes, n=1000, size=64, device=None, generator=None, samples=2):
        """n items: a uniformly random mesh of ``meshes`` each (drawn first), then n Haar poses
        (random_group_matrices), then the renders."""
        meshes = _mesh_set(meshes, device)
        names = torch.randint(meshes.K, (n,), device=meshes.device, generator=generator)
        g = random_group_matrices(n, device=meshes.device, generator=generator)
        return cls(tensors=(names, g, _render_mesh_chunked(g, meshes, names, size, samples)))

    def __len__(self):
        return self.tensors[0].shape[0]

    def __getitem__(self, idx):
        names, g, x = self.tensors
        return names[idx], g[idx], x[idx]

    def save(self, path='data/meshes.pt'):
        torch.save(tuple(t.cpu() for t in self.tensors), path)

    @staticmethod
    def prep_batch(batch):
        return batch
