"""The painter rule of a scene (several meshes over one frame, dynaboa_amd/csrc/render.hip: the scene entry) as a chain of
tests/render_ref.render calls: there is no depth between meshes, the mesh listed later is on top wherever it covers a pixel."""
import numpy as np

import render_ref as RR


def render_scene(meshes, faces, H, W, background=None):
    """meshes: [(verts (V, 3), cam (4,), color (3,)), ...] in painter order.  -> (image (H, W, 3) uint8, mesh_id (H, W) int32,
    face_id (H, W) int32): mesh_id is the LAST listed mesh whose own face_id is >= 0 at the pixel, face_id that mesh's; -1 where no
    mesh covers the pixel."""
    img = np.zeros((H, W, 3), np.uint8) if background is None else np.array(background, np.uint8)
    mesh_id = np.full((H, W), -1, np.int32)
    face_id = np.full((H, W), -1, np.int32)
    for k, (verts, cam, color) in enumerate(meshes):
        r = RR.render(verts, faces, cam, H, W, img, color)
        cov = r.face_id >= 0
        mesh_id[cov] = k
        face_id[cov] = r.face_id[cov]
        img = r.image
    return img, mesh_id, face_id
