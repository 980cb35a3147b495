"""Generate tests/golden/panda_collision_meshes.npz: the vertex sets of the Panda's collision meshes (the reference's
urdf/franka_panda/meshes/collision/*.obj) and the <collision><origin> that places each of them on its link
(urdf/franka_panda/panda.urdf), one entry per link with a collision mesh, in the URDF's link order.  DATA, read by
tests/test_link_geometry_data.py to check that robots/panda_link_capsules.json contains every mesh vertex.

    python tests/golden/make_panda_collision_meshes.py <reference checkout>

Keys: "links" (link names), "<link>.vertices" [n, 3] float64 (mesh coordinates, as written in the .obj),
"<link>.xyz" [3] and "<link>.rpy" [3] float64 (the collision origin; zeros where the URDF gives none).
"""
import os
import sys
from xml.etree import ElementTree

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from riemannian_motion_policies_amd.urdf import _floats  # noqa: E402


def read_obj_vertices(path):
    v = [list(map(float, line.split()[1:4])) for line in open(path) if line.startswith("v ")]
    return np.asarray(v, dtype=np.float64)


def main(reference):
    urdf = os.path.join(reference, "urdf", "franka_panda", "panda.urdf")
    root = ElementTree.parse(urdf).getroot()
    out, links = {}, []
    for link in root.findall("link"):
        col = link.find("collision")
        mesh = col.find("geometry").find("mesh") if col is not None else None
        if mesh is None:
            continue
        name = link.attrib["name"]
        origin = col.find("origin")
        out[f"{name}.vertices"] = read_obj_vertices(
            os.path.join(os.path.dirname(urdf), mesh.attrib["filename"].replace("package://", "")))
        out[f"{name}.xyz"] = np.asarray(_floats(origin.attrib.get("xyz") if origin is not None else None), dtype=np.float64)
        out[f"{name}.rpy"] = np.asarray(_floats(origin.attrib.get("rpy") if origin is not None else None), dtype=np.float64)
        links.append(name)
        print(f"{name:18s} {len(out[f'{name}.vertices']):4d} vertices")
    dst = os.path.join(HERE, "panda_collision_meshes.npz")
    np.savez_compressed(dst, links=np.array(links), **out)
    print("wrote", dst)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
