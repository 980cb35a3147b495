"""Write tests/golden/robot_inertials.npz: the raw <inertial> data of every link of the reference's two robots.

usage: python tests/golden/make_robot_inertials.py <reference checkout>

Reads <ref>/urdf/franka_panda/panda.urdf and <ref>/urdf/TwoJointRobot_wo_fixedJoints.urdf.  Per robot (prefix "panda" /
"two_joint"): <prefix>.links (names, document order), <prefix>.mass [n], <prefix>.xyz [n, 3], <prefix>.rpy [n, 3] (the inertial
origin; 0 where absent), <prefix>.inertia6 [n, 6] = (ixx, iyy, izz, ixy, ixz, iyz) as written.  Links without an <inertial> are
not listed.  The package's kinematics-only URDFs carry no inertials; the tests feed these to urdf.inertial_table."""
import os
import sys
from xml.etree import ElementTree

import numpy as np

ROBOTS = {"panda": "urdf/franka_panda/panda.urdf", "two_joint": "urdf/TwoJointRobot_wo_fixedJoints.urdf"}


def _vec(el, key):
    return [float(v) for v in el.attrib.get(key, "0 0 0").split()] if el is not None else [0.0, 0.0, 0.0]


def main(ref: str) -> None:
    out = {}
    for prefix, rel in ROBOTS.items():
        root = ElementTree.parse(os.path.join(ref, rel)).getroot()
        names, mass, xyz, rpy, inertia = [], [], [], [], []
        for link in root.findall("link"):
            inr = link.find("inertial")
            if inr is None:
                continue
            names.append(link.attrib["name"])
            mass.append(float(inr.find("mass").attrib["value"]))
            origin = inr.find("origin")
            xyz.append(_vec(origin, "xyz"))
            rpy.append(_vec(origin, "rpy"))
            i = inr.find("inertia").attrib
            inertia.append([float(i.get(k, "0")) for k in ("ixx", "iyy", "izz", "ixy", "ixz", "iyz")])
        out[f"{prefix}.links"] = np.array(names)
        out[f"{prefix}.mass"] = np.array(mass, np.float64)
        out[f"{prefix}.xyz"] = np.array(xyz, np.float64).reshape(-1, 3)
        out[f"{prefix}.rpy"] = np.array(rpy, np.float64).reshape(-1, 3)
        out[f"{prefix}.inertia6"] = np.array(inertia, np.float64).reshape(-1, 6)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "robot_inertials.npz")
    np.savez(dst, **out)
    print(f"wrote {dst}: " + ", ".join(f"{p} {len(out[p + '.links'])} links" for p in ROBOTS))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
