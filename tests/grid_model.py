"""Numpy restatement of the selection grid's header (srb_grid_build_kernel, csrc/srb_select.hip) and of the gate
in front of the ring search (knn_select_k, csrc/srb_knn.h).

An input check, not a kernel check: a test that forces the grid cannot see from outside whether a query went
through the ring search or fell back to the brute-force scan, so tests/test_knn_grid_small.py asks this model
which of its queries reach the grid.  The selected rows themselves are compared with oracle.select_idx."""
import numpy as np

CELLS = 16384          # SRB_GRID_CELLS
GATE = 64.0            # cells a query may lie outside the grid and still search it


def header(xy):
    """The header the build stores for a table whose rows' positions are xy [n][2]: dict(ok, x0, y0, h, inv_h,
    nx, ny, n); ok = 0 (no finite row) carries nothing else."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    fin = np.isfinite(xy).all(1)
    if not fin.any():
        return dict(ok=0)
    x0, y0 = xy[fin].min(0)
    x1, y1 = xy[fin].max(0)
    with np.errstate(over="ignore", invalid="ignore"):
        W, H = np.float64(x1 - x0), np.float64(y1 - y0)
        target = np.float64(min(max(len(xy) // 2, 1), CELLS))
        h = np.sqrt(np.fmax(W * H, 1e-300) / target)
        if not (h > 0.0) or not np.isfinite(h):
            h = np.float64(1.0)
        h = np.fmax(h, np.fmax(W, H) / 4096.0)
        nx, ny = int(W / h) + 1, int(H / h) + 1
        while nx * ny > CELLS:
            h = h * 1.25
            nx, ny = int(W / h) + 1, int(H / h) + 1
        return dict(ok=1, x0=x0, y0=y0, h=h, inv_h=np.float64(1.0) / h, nx=nx, ny=ny, n=int(fin.sum()))


def cell(g, px, py):
    """(fx, fy): the floating-point cell coordinates of a query, as the gate computes them."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.floor((np.float64(px) - g["x0"]) * g["inv_h"]), np.floor((np.float64(py) - g["y0"]) * g["inv_h"]))


def through_grid(g, px, py, K, own_row=False):
    """True when knn_select_k searches the grid for this query, False when it falls back to the scan: the grid
    holds K rows (plus one for the agent's own row in a neighbour table) and the query lies within 64 cells."""
    if not g["ok"] or K <= 0:
        return False
    fx, fy = cell(g, px, py)
    keff = K + (1 if own_row else 0)
    return bool(g["n"] >= keff and fx > -GATE and fy > -GATE and fx < g["nx"] + GATE and fy < g["ny"] + GATE)
