"""Shared inputs of the fleet-scan tests (tests/test_lidar_fleet_cpu.py, tests/test_gpu_lidar_fleet.py): a fleet on a
square floor with boxes and world circles, every robot's body centred at its body offset, plus the restatement's answer,
computed once per case and left unchanged."""
import functools
import math

import numpy as np

from lidar_fleet_reference import fleet_scan_ref

RANGE, OFFSET, BODY_OFFSET, HEIGHT = 9.0, (0.4, 0.15), (0.25, -0.1), 0.02
NBOX, NCIRCLE = 60, 5
# (B, R, P, self0, arena half-width, (least, largest radius)): the smallest shapes at which the chunking (P below,
# at and above one block of bodies; R below, at and above one block of rays), the tie-break and self0 can go wrong;
# the last is dense: every robot has more bodies in range than the kernel's list holds
PARITY_CASES = [(37, 1, 37, 0, 6.0, (0.3, 0.6)), (37, 64, 37, 0, 6.0, (0.3, 0.6)), (37, 257, 42, 2, 6.0, (0.3, 0.6)),
                (1031, 64, 1031, 0, 24.0, (0.3, 0.6)), (700, 64, 1031, 165, 4.0, (0.025, 0.05))]
DENSE_MIN_IN_RANGE = 900


def body_centres(pose, body_offset=BODY_OFFSET):
    c, s = np.cos(pose[:, 2]), np.sin(pose[:, 2])
    return np.stack([pose[:, 0] + body_offset[0] * c - body_offset[1] * s,
                     pose[:, 1] + body_offset[0] * s + body_offset[1] * c], axis=1)


def fleet_world(rng, B, P, self0, arena, radii, stride=8):
    """pose (B, stride), boxes (NBOX, 4), circles (NCIRCLE, 3), centres (P, 3), radius (P,): robot b's body is
    self0 + b; the other bodies stand anywhere on the floor.  Box sides are 1 .. 10 % of the arena's half-width."""
    pose = rng.normal(size=(B, stride))
    pose[:, :2] = rng.uniform(-arena, arena, (B, 2))
    pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
    boxes = np.concatenate([rng.uniform(-arena, arena, (NBOX, 2)), rng.uniform(0.01, 0.1, (NBOX, 2)) * arena], 1)
    circles = np.concatenate([rng.uniform(-arena, arena, (NCIRCLE, 2)), rng.uniform(0.02, 0.08, (NCIRCLE, 1)) * arena], 1)
    centres = np.concatenate([rng.uniform(-arena, arena, (P, 2)), np.zeros((P, 1))], 1)
    own = self0 + np.arange(B)
    ok = (own >= 0) & (own < P)
    centres[own[ok], :2] = body_centres(pose)[ok]
    radius = rng.uniform(radii[0], radii[1], P)
    return pose, boxes, circles, centres, radius


@functools.lru_cache(maxsize=None)
def parity_case(n):
    """inputs and the restatement's answer of PARITY_CASES [n]; do not modify the arrays"""
    B, R, P, self0, arena, radii = PARITY_CASES[n]
    rng = np.random.default_rng(B * 1000 + R)
    pose, boxes, circles, centres, radius = fleet_world(rng, B, P, self0, arena, radii)
    ref = fleet_scan_ref(pose, R, -math.pi, math.pi, RANGE, OFFSET, HEIGHT, boxes, circles, centres, radius, self0)
    return dict(B=B, R=R, P=P, self0=self0, pose=pose, boxes=boxes, circles=circles, centres=centres, radius=radius,
                ref=ref)


def in_range_counts(case):
    """(B,) bodies within range + r of each robot's sensor, the robot's own left out"""
    from lidar_reference import sensor_origin
    pose = case["pose"]
    ox, oy = sensor_origin(pose[:, 0], pose[:, 1], pose[:, 2], OFFSET)
    d = np.hypot(ox[:, None] - case["centres"][None, :, 0], oy[:, None] - case["centres"][None, :, 1])
    inr = d <= RANGE + case["radius"][None, :]
    own = case["self0"] + np.arange(case["B"])
    ok = (own >= 0) & (own < case["P"])
    inr[np.flatnonzero(ok), own[ok]] = False
    return inr.sum(axis=1)


def excluded(ref):
    return ref["near"] | ref["sensitive"] | ref["ambiguous"]


def outcome_shares(ref):
    """shares of the rays that end on a body, on the static world with a body hit behind it, on nothing"""
    own = ref["owner"]
    return (own >= 0).mean(), ((own == -2) & ref["body_hits"]).mean(), (own == -1).mean()


def sensor_centred(rng, B, arena, radii=(0.3, 0.6), stride=8):
    """a fleet whose bodies are centred on the sensors (body offset = sensor offset): every robot's own body contains
    its sensor, so appending the bodies to the world's circles gives the plain scan the same answer"""
    from lidar_reference import sensor_origin
    pose, boxes, circles, centres, radius = fleet_world(rng, B, B, 0, arena, radii, stride)
    ox, oy = sensor_origin(pose[:, 0], pose[:, 1], pose[:, 2], OFFSET)
    centres[:, 0], centres[:, 1] = ox, oy
    allc = np.concatenate([circles, np.stack([ox, oy, radius], axis=1)], 0)
    return pose, boxes, circles, centres, radius, allc
