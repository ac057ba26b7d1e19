"""The scene fact "a path can go on from Lambertian surfaces only" -- every object Lambertian, or Emissive with a non-zero emission
(a hit there ends the path) -- is decided on the host when the records of an upload are built (ptscene::build) and travels in
the scene view (SceneView::lambert_surfaces).  Here, without a device (pt_debug_lambert_surfaces with no context): it is what the
object list implies, for every scene of the GPU test.

pt_scene_update keeps object count and shape tags and nothing else: a material may change under it.  Every scene_set builds the
records anew, the flag with them; what can be pinned without a device is that the updated list is one pt_scene_update accepts and
that its records carry the other flag (the context following it: tests/test_gpu_lambert_surfaces.py)."""
import ctypes as C

import pytest

import lambert_surfaces_cases as cases


def _implied(objs):
    """the definition, restated on the object list (an Emissive emits when the f32 length of its emission is > 0)"""
    return all(o.mat_tag == cases.LAMBERT or _emits(o) for o in objs)


def _emits(o):
    import numpy as np
    p = [np.float32(o.mat[k]) for k in range(3)]
    return o.mat_tag == cases.EMISSIVE and np.sqrt(np.float32(sum(float(x) * float(x) for x in p))) > 0


@pytest.mark.parametrize("name", cases.NAMES)
def test_flag_is_what_the_object_list_implies(pt, name):
    objs, lambert, only, lights = cases.scene(pt, name)
    assert lambert == _implied(objs), "the case table contradicts itself"
    assert sum(bool(_emits(o)) for o in objs) == lights
    assert pt.scene_lambert_surfaces(objs) == lambert
    assert pt.scene_spheres_only(objs) == only


def test_the_light_made_lambertian_keeps_the_flag_and_has_no_light(pt):
    """... so k_paths_regen<MIS, diffuse> still takes its generic loop: the fast one asks for exactly one light"""
    objs, lambert, only, lights = cases.scene(pt, "c2_no_light")
    assert lambert and only and lights == 0 and pt.scene_lambert_surfaces(objs)


def test_a_material_change_is_an_update_and_changes_the_flag(pt):
    base = cases.scene(pt, "c2")[0]
    for name in ("c2_black_emissive", "c2_oren_nayar", "c2_mirror", "c2_no_light"):
        objs, lambert, _, _ = cases.scene(pt, name)
        assert len(objs) == len(base) and all(a.shape_tag == b.shape_tag for a, b in zip(objs, base))   # what pt_scene_update checks
        assert pt.scene_lambert_surfaces(objs) == lambert
    assert pt.scene_lambert_surfaces(base)


def test_a_dim_emissive_is_a_light_and_a_black_one_is_not(pt):
    objs = cases.scene(pt, "c2")[0]
    o = objs[8]
    cases._set_mat(o, cases.EMISSIVE, (0.0, 1e-10, 0.0))        # squared length 1e-20: > 0 in f32, it emits
    assert pt.scene_lambert_surfaces(objs)
    cases._set_mat(o, cases.EMISSIVE, (0.0, 1e-30, 0.0))        # squared length 1e-60: 0 in f32, as the upload evaluates it
    assert not pt.scene_lambert_surfaces(objs)


def test_edges(pt):
    lib = pt._lib.lib()
    v = C.c_uint32(7)
    assert lib.pt_debug_lambert_surfaces(None, None, 0, C.byref(v)) == 0 and v.value == 1     # no object: nothing contradicts it
    assert lib.pt_debug_lambert_surfaces(None, None, 3, C.byref(v)) != 0                      # objects announced, none given
    objs = cases.scene(pt, "c2")[0]
    assert lib.pt_debug_lambert_surfaces(None, objs, len(objs), None) != 0
    objs[0].mat_tag = 9
    assert lib.pt_debug_lambert_surfaces(None, objs, len(objs), C.byref(v)) != 0              # a bad tag: the upload's own refusal
    # position does not matter: first, last, alone
    for where in (0, len(objs) - 1):
        objs = cases.scene(pt, "c2")[0]
        cases._set_mat(objs[where], cases.OREN_NAYAR, (0.5, 0.5, 0.5, 0.3))
        assert not pt.scene_lambert_surfaces(objs)
    one = pt.make_objects([(0, (0, 0, -2, 0.5), cases.MIRROR, (0.1, 0.9, 0.9, 0.9, 1.0, 1.5))])
    assert not pt.scene_lambert_surfaces(one)
    assert pt.scene_lambert_surfaces(pt.make_objects([(0, (0, 0, -2, 0.5), cases.EMISSIVE, (1.0, 1.0, 1.0))]))
