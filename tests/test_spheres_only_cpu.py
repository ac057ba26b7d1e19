"""The scene-shape fact "the scan array is one run of at most 16 spheres at offset 0, first object 0" is decided on the host when
the records of an upload are built (ptscene::build) and travels in the scene view (SceneView::spheres_only).  Here, without a
device (pt_debug_spheres_only with no context): it is what the object list implies, for every scene of the GPU test."""
import ctypes as C

import pytest

import spheres_only_cases as cases


@pytest.mark.parametrize("name", cases.NAMES)
def test_flag_is_what_the_object_list_implies(pt, name):
    objs, only, _ = cases.scene(pt, name)
    spheres = sum(o.shape_tag == 0 for o in objs)
    assert only == (spheres == len(objs) and 1 <= len(objs) <= 16), "the case table contradicts itself"
    assert pt.scene_spheres_only(objs) == only


def test_edges(pt):
    lib = pt._lib.lib()
    v = C.c_uint32(7)
    assert lib.pt_debug_spheres_only(None, None, 0, C.byref(v)) == 0 and v.value == 0       # no object: no run
    assert lib.pt_debug_spheres_only(None, None, 3, C.byref(v)) != 0                        # objects announced, none given
    objs, _, _ = cases.scene(pt, "c2")
    assert lib.pt_debug_spheres_only(None, objs, len(objs), None) != 0
    # a triangle in front, behind, and alone
    tri = pt.make_objects([(1, (0, 0, -2, 1, 0, -2, 0, 1, -2), 0, (0.5, 0.5, 0.5))])[0]
    one = list(objs)
    assert not pt.scene_spheres_only((pt._lib.PtObject * 11)(tri, *one))
    assert not pt.scene_spheres_only((pt._lib.PtObject * 11)(*one, tri))
    assert not pt.scene_spheres_only((pt._lib.PtObject * 1)(tri))
    assert pt.scene_spheres_only((pt._lib.PtObject * 1)(one[0]))
