"""Scenes of tests/test_gpu_lambert_surfaces.py and tests/test_lambert_surfaces_cpu.py: scene 2 (ten diffuse spheres, one of them the
light) and what the sphere-hit, Lambert-only vertex stage of k_paths_regen<MIS, diffuse> must tell apart from it.
name -> (objects, lambert_surfaces the upload must record, spheres_only, lights)."""
import spheres_only_cases as so

LIGHT = so.LIGHT
LAMBERT, EMISSIVE, MIRROR, OREN_NAYAR = 0, 1, 2, 3


def _set_mat(o, tag, values):
    o.mat_tag = tag
    for k in range(6):
        o.mat[k] = float(values[k]) if k < len(values) else 0.0


def scene(pt, name):
    """-> (PtObject array, lambert_surfaces, spheres_only, lights)"""
    if name == "none":
        return (pt._lib.PtObject * 0)(), True, False, 0
    if name == "c1":
        objs = pt.builtin_scene(1)
        assert any(o.mat_tag == MIRROR for o in objs)
        return objs, False, False, 2
    objs = so._copy(pt, pt.builtin_scene(2))
    lambert, only, lights = True, True, 1
    if name == "c2_oren_nayar":
        _set_mat(objs[6], OREN_NAYAR, (0.8, 0.8, 0.8, 0.5))           # albedo, sigma
        lambert = False
    elif name == "c2_mirror":
        _set_mat(objs[7], MIRROR, (0.1, 0.9, 0.9, 0.9, 1.0, 1.5))     # roughness, colour, metallic, ior
        lambert = False
    elif name == "c2_black_emissive":
        # Emissive that does not emit: no light, no end of the path -- it goes on with f = 0, pdf = 1, wo = n
        _set_mat(objs[8], EMISSIVE, (0.0, 0.0, 0.0))
        lambert = False
    elif name == "c2_no_light":
        _set_mat(objs[LIGHT], LAMBERT, (0.8, 0.8, 0.8))
        lights = 0
    elif name == "c2_two":
        objs = so.c2_with_n_spheres(pt, 2)                             # the light and one sphere
    elif name == "c2_sixteen":
        objs = so.c2_with_n_spheres(pt, 16)
    elif name == "c2_triangle_for_sphere":
        objs = list(so.scene(pt, name)[0])
        only = False
    else:
        assert name == "c2", name
    return so._array(pt, objs), lambert, only, lights


NAMES = ["c2", "c2_oren_nayar", "c2_mirror", "c2_black_emissive", "c2_no_light", "c1", "none", "c2_two", "c2_sixteen", "c2_triangle_for_sphere"]
