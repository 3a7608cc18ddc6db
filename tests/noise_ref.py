"""float64 numpy restatement of the noise-HPO objective, the checker of tests/test_hpo_host.py (pinned there to the
reference driver's own lines through tests/golden/noise_objective_*.npz, variant (ii): the driver's arithmetic on the
fp16 tensors upcast to float64) and of tests/test_gpu_noise_hpo.py.

  sums        per step and group of images: S (a - b)^2, A = S |a|, B = S |b|, S (a / max(A, 1e-12) - b / max(B,
              1e-12))^2 -- what sdmoe_noise_distance writes; the divisions element by element, as F.normalize does
  distances   their square roots: torch.norm(a - b) and the distance of the F.normalize(p = 1)'d vectors
  objective   the driver's bookkeeping over samples: per-step means of l2, their mean (the trial's score), per-sample
              means of l1n
"""
import numpy as np

EPS = 1e-12  # torch.nn.functional.normalize's clamp


def sums(a, b, img_group=None, ngroups=1):
    """a, b: [T, nimg, ...] arrays (any float dtype; the elements of image i are a[t, i].ravel()) -> float64
    [T, ngroups, 4]; image i belongs to group img_group[i] (None: all group 0)."""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    T, nimg = a.shape[:2]
    groups = [0] * nimg if img_group is None else [int(g) for g in img_group]
    out = np.zeros((T, ngroups, 4), dtype=np.float64)
    for t in range(T):
        for g in range(ngroups):
            imgs = [i for i in range(nimg) if groups[i] == g]
            if not imgs:
                continue
            x, y = a[t, imgs].reshape(-1), b[t, imgs].reshape(-1)
            A, B = np.abs(x).sum(), np.abs(y).sum()
            d = x / max(A, EPS) - y / max(B, EPS)
            out[t, g] = [((x - y) ** 2).sum(), A, B, (d * d).sum()]
    return out


def distances(a, b, img_group=None, ngroups=1):
    """(l2 [T, G], l1n [T, G])."""
    s = sums(a, b, img_group, ngroups)
    return np.sqrt(s[:, :, 0]), np.sqrt(s[:, :, 3])


def objective(l2, l1n):
    """l2, l1n: [samples, T] -> (per-step mean of l2 over the samples [T], its mean over the steps, per-sample mean of
    l1n over the steps [samples])."""
    l2, l1n = np.asarray(l2, dtype=np.float64), np.asarray(l1n, dtype=np.float64)
    step_avg = l2.sum(0) / l2.shape[0]
    return step_avg, step_avg.sum() / l2.shape[1], l1n.sum(1) / l1n.shape[1]
