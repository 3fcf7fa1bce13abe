"""nav/quad_helpers.py:186-258: the rotation step of the planner's start state and the A* search of its initial path."""
import heapq

import numpy as np
import torch

from .math_utils import skew_matrix


def next_rotation(R, omega, dt):
    """Propagate the rotation matrix by the exponential map of omega * dt (quad_helpers.py:186-199)."""
    angle = omega * dt
    theta = torch.norm(angle, p=2)
    eye = torch.eye(3, dtype=R.dtype, device=R.device)
    if theta == 0:
        exp_i = eye
    else:
        angle_norm = angle / theta
        K = skew_matrix(angle_norm)
        exp_i = eye + torch.sin(theta) * K + (1 - torch.cos(theta)) * torch.matmul(K, K)
    return R @ exp_i


def astar(occupied, start, goal):
    """Six-neighbour A* on the boolean grid `occupied` from `start` to `goal` (index tuples) -> list of index tuples
    (quad_helpers.py:201-258): the same heap entries (f, node), ties broken by the node tuple, and the same `node not in open_heap`
    check, so the path is the reference's.  An occupied start or goal raises AssertionError, no path ValueError.
    A device tensor is read back once instead of once per visited cell."""
    if isinstance(occupied, torch.Tensor):
        occupied = occupied.detach().cpu().numpy()
    occupied = np.asarray(occupied)

    def heuristic(a, b):
        return np.sqrt((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2 + (b[2] - a[2]) ** 2)

    def inbounds(point):
        for x, size in zip(point, occupied.shape):
            if x < 0 or x >= size:
                return False
        return True

    neighbors = [(1, 0, 0), (-1, 0, 0),
                 (0, 1, 0), (0, -1, 0),
                 (0, 0, 1), (0, 0, -1)]

    close_set = set()
    came_from = {}
    gscore = {start: 0}

    assert not occupied[start]
    assert not occupied[goal]

    open_heap = []
    heapq.heappush(open_heap, (heuristic(start, goal), start))

    while open_heap:
        current = heapq.heappop(open_heap)[1]

        if current == goal:
            data = []
            while current in came_from:
                data.append(current)
                current = came_from[current]
            assert current == start
            data.append(current)
            return list(reversed(data))

        close_set.add(current)

        for i, j, k in neighbors:
            neighbor = (current[0] + i, current[1] + j, current[2] + k)
            if not inbounds(neighbor):
                continue
            if occupied[neighbor]:
                continue

            tentative_g_score = gscore[current] + 1
            if tentative_g_score < gscore.get(neighbor, float("inf")):
                came_from[neighbor] = current
                gscore[neighbor] = tentative_g_score

                fscore = tentative_g_score + heuristic(neighbor, goal)
                node = (fscore, neighbor)
                if node not in open_heap:
                    heapq.heappush(open_heap, node)

    raise ValueError("Failed to find path!")
