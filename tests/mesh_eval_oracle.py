"""The PVE rule of DESIGN.md 4c restated in numpy float64 (not imported by the product): the per-vertex error of two meshes, each
centred at its own pelvis, and the same after a Procrustes alignment of all V raw points."""
import numpy as np


def similarity_transform(S1, S2):
    """(scale, R, t) of the best similarity transform of the points S1 [V,3] onto S2 [V,3], det R = +1."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    mu1, mu2 = S1.mean(0), S2.mean(0)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum()
    K = X1.T @ X2
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    scale = np.trace(R @ K) / var1
    return scale, R, mu2 - scale * (R @ mu1)


def vertex_errors(pred_vertices, gt_vertices, pelvis_row):
    """pred_vertices, gt_vertices [B,V,3], pelvis_row [V] -> (pve [B], pa_pve [B]) float64, in the unit of the inputs."""
    P, G, w = np.asarray(pred_vertices, np.float64), np.asarray(gt_vertices, np.float64), np.asarray(pelvis_row, np.float64)
    pve, pa = np.zeros(len(P)), np.zeros(len(P))
    for b in range(len(P)):
        d = (P[b] - w @ P[b]) - (G[b] - w @ G[b])
        pve[b] = np.sqrt((d ** 2).sum(-1)).mean()
        s, R, t = similarity_transform(P[b], G[b])
        pa[b] = np.sqrt(((s * P[b] @ R.T + t - G[b]) ** 2).sum(-1)).mean()
    return pve, pa
