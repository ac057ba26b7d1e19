"""Scenes of tests/test_gpu_spheres_only.py and tests/test_spheres_only_cpu.py: scene 2 (ten diffuse spheres, one of them the
light) and what the spheres-only form of k_paths_regen<MIS, diffuse> must tell apart from it.  name -> (objects, spheres_only the
upload must record, lights)."""

LIGHT = 5                 # scene 2's sphere light (pt_scenes.cpp)
CUTS = (1, 2, 3, 4, 5, 7, 8, 9, 16)     # every remainder of the groups of four, two and one, and the count limit


def _copy(pt, objs):
    return [pt._lib.PtObject.from_buffer_copy(o) for o in objs]


def _array(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def _small_spheres(pt, n):
    return pt.make_objects([(0, (-0.6 + 0.2 * j, -0.5, -1.8, 0.08), 0, (0.7, 0.6, 0.5)) for j in range(n)])


def _triangle_like(pt, o, verts):
    """a triangle with the material of object o"""
    tri = pt.make_objects([(1, verts, 0, (0.5, 0.5, 0.5))])[0]
    tri.mat_tag = o.mat_tag
    for k in range(6):
        tri.mat[k] = o.mat[k]
    return tri


def c2_with_n_spheres(pt, n):
    """scene 2 cut to (or filled up to) n spheres, the light among them: one light, spheres only"""
    objs = _copy(pt, pt.builtin_scene(2))
    if n <= len(objs):
        return [objs[LIGHT]] + [o for i, o in enumerate(objs) if i != LIGHT][:n - 1]
    return objs + list(_small_spheres(pt, n - len(objs)))


def scene(pt, name):
    """-> (PtObject array, spheres_only, lights)"""
    objs = _copy(pt, pt.builtin_scene(2))
    assert len(objs) == 10 and all(o.shape_tag == 0 for o in objs)
    assert objs[LIGHT].mat_tag == 1 and sum(o.mat_tag == 1 for o in objs) == 1 and all(o.mat_tag <= 1 for o in objs)
    only, lights = True, 1
    if name.startswith("c2_cut_"):
        n = int(name[len("c2_cut_"):])
        objs = c2_with_n_spheres(pt, n)
        only = n <= 16
    elif name == "c2_triangle_for_sphere":
        # two runs (spheres 0 .. 8, one triangle): the generic walk
        objs[9] = _triangle_like(pt, objs[9], (-0.5, -0.6, -2.4, 0.1, -0.6, -2.4, -0.2, 0.1, -2.2))
        only = False
    elif name == "c2_triangle_light":
        objs[LIGHT] = pt.make_objects([(1, (-0.3, 0.79, -2.3, 0.3, 0.79, -2.3, 0.3, 0.79, -1.7), 1, (15.0, 15.0, 15.0))])[0]
        only = False
    elif name == "c2_two_lights":
        objs.append(pt.make_objects([(0, (0.55, 0.2, -2.3, 0.1), 1, (10.0, 6.0, 2.0))])[0])
        lights = 2
    elif name == "c2_plus_triangle":
        objs.append(_triangle_like(pt, objs[0], (-0.5, -0.6, -2.4, 0.1, -0.6, -2.4, -0.2, 0.1, -2.2)))
        only = False
    elif name == "c2_moved":
        objs[2].shape[0] += 0.125
        objs[2].shape[1] += 0.0625
    else:
        assert name == "c2", name
    return _array(pt, objs), only, lights


NAMES = (["c2"] + [f"c2_cut_{n}" for n in CUTS] + ["c2_cut_17", "c2_triangle_for_sphere", "c2_triangle_light", "c2_two_lights",
                                                     "c2_plus_triangle", "c2_moved"])
