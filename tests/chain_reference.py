"""Reference kinematics of a serial URDF chain (tests only; numpy, scipy and the XML reader of the standard library --
nothing of the package, of the oracle or of oracle/nlp_numpy.py).

A frame is the product of homogeneous 4 x 4 matrices  T = prod_j  Origin_j  Motion_j(q_j):  Origin_j the joint's
`<origin>` (translation xyz, rotation ``Rotation.from_euler("xyz", rpy)``: URDF's fixed-axis roll, pitch, yaw),
Motion_j a rotation ``Rotation.from_rotvec(axis q)`` about the normalised `<axis>` (revolute, continuous) or a
translation ``axis q`` (prismatic).  URDF defaults: no `<origin>` = identity, no `<axis>` = (1, 0, 0).

Derivatives of a frame's position are central differences at h, h/2 and h/4, extrapolated twice (Richardson: the error
terms h^2 and h^4 cancel), returned with their own uncertainty u: the max-norm of the difference between the last two
extrapolated values -- as hessian_reference.py does for the stage Hessian.
"""
import xml.etree.ElementTree as ET

import numpy as np
from scipy.spatial.transform import Rotation

H1 = 2e-2   # largest step of the three, first derivatives
H2 = 5e-2   # second derivatives


def read_chain(urdf_path, end_link):
    """Joints from the URDF's root to ``end_link``, in order: dicts (type, xyz, rpy, axis [unit], child)."""
    robot = ET.parse(urdf_path).getroot()
    above = {j.find("child").get("link"): j for j in robot.findall("joint")}
    vec = lambda el, key, dflt: np.array([float(v) for v in el.get(key).split()]) if el is not None and el.get(key) else np.array(dflt, dtype=float)
    out, link = [], end_link
    while link in above:
        j = above[link]
        axis = vec(j.find("axis"), "xyz", (1.0, 0.0, 0.0))
        out.append(dict(type=j.get("type"), xyz=vec(j.find("origin"), "xyz", (0.0, 0.0, 0.0)),
                        rpy=vec(j.find("origin"), "rpy", (0.0, 0.0, 0.0)), axis=axis / np.linalg.norm(axis), child=link))
        link = j.find("parent").get("link")
    return out[::-1]


def _hom(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def frames(chain, q):
    """4 x 4 matrix of every joint's child frame at q (q[i]: the i-th joint of the chain; none of them fixed)."""
    T, out = np.eye(4), []
    for j, qj in zip(chain, q):
        T = T @ _hom(Rotation.from_euler("xyz", j["rpy"]).as_matrix(), j["xyz"])
        if j["type"] in ("revolute", "continuous"):
            T = T @ _hom(Rotation.from_rotvec(j["axis"] * qj).as_matrix(), np.zeros(3))
        elif j["type"] == "prismatic":
            T = T @ _hom(np.eye(3), j["axis"] * qj)
        else:
            raise ValueError(j["type"])
        out.append(T.copy())
    return out


def position(chain, q, frame):
    return frames(chain, q)[frame][:3, 3].copy()


def _richardson(central, h):
    d0, d1, d2 = (central(h / s) for s in (1.0, 2.0, 4.0))
    r0 = (4.0 * d1 - d0) / 3.0
    r1 = (4.0 * d2 - d1) / 3.0
    r2 = (16.0 * r1 - r0) / 15.0
    return r2, float(np.abs(r2 - r1).max())


def jacobian(chain, q, frame, h=H1):
    """(J [3, n], u): d position / dq of a frame and its uncertainty."""
    q = np.array(q, dtype=np.float64)
    n = q.size

    def central(hh):
        J = np.zeros((3, n))
        for a in range(n):
            qp = q.copy(); qm = q.copy()
            qp[a] += hh; qm[a] -= hh
            J[:, a] = (position(chain, qp, frame) - position(chain, qm, frame)) / (qp[a] - qm[a])
        return J

    return _richardson(central, h)


def second_derivatives(chain, q, frame, h=H2):
    """(D [3, n, n], u): d2 position / dq_a dq_b of a frame (symmetric in a, b) and its uncertainty."""
    q = np.array(q, dtype=np.float64)
    n = q.size

    def central(hh):
        D = np.zeros((3, n, n))
        p0 = position(chain, q, frame)
        for a in range(n):
            for b in range(a, n):
                if a == b:
                    qp = q.copy(); qm = q.copy()
                    qp[a] += hh; qm[a] -= hh
                    D[:, a, a] = (position(chain, qp, frame) - 2.0 * p0 + position(chain, qm, frame)) / (hh * hh)
                else:
                    v = 0.0
                    for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                        qq = q.copy()
                        qq[a] += sa * hh; qq[b] += sb * hh
                        v = v + sa * sb * position(chain, qq, frame)
                    D[:, a, b] = D[:, b, a] = v / (4.0 * hh * hh)
        return D

    return _richardson(central, h)
