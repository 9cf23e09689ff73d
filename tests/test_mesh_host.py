"""Triangle meshes from depth (gp_depth_mesh), the host half: genpercept_amd/mesh.py (vectorised numpy) bit-equal to plain Python loops over
cells and nodes written here from the definition; tests/mesh_check.cpp, a stand-alone CPU program over the kernels' own arithmetic
(csrc/depth_mesh_math.h, contraction off, under AddressSanitizer and UBSan), bit-equal to the host route; what the definition is for -- a
fronto-parallel plane is fully meshed, no face crosses a depth step, one foreground corner leaves the one background triangle, every face
looks at the camera and the surface is a manifold with consistent orientation; indices, offsets, empty images and degenerate grids; the .glb
and .ply writers read back by parsers of their own; the header, the two libraries and the ctypes table carry the new entries; their
argument checks (they come before the first HIP call, so they run without a GPU).  There is no tolerance in this file."""
import ctypes as C
import io
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import libs as _libs, same_bits  # noqa: E402
from test_geometry_host import PLANES, random_case  # noqa: E402

NAMES = ("gp_depth_mesh_workspace", "gp_depth_mesh")
MESH = ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "vertex_index", "faces")
OFFSETS = ("vertex_offsets", "face_offsets")
f32, f64 = np.float32, np.float64
SCENES = [(9, 13), (17, 23), (12, 12), (5, 23)]


# ---- the definition as plain loops ---------------------------------------------------------------------------------------------------------------
def loops_linked(kp, zp, kq, zq, cut):
    if not (kp and kq):
        return False
    d = abs(zp - zq)
    m = min(zp, zq)
    return d <= cut * m


def loops_mesh(xyz, normal, keep, image, stride, cut):
    """One image, literally: Python floats (IEEE float64, one operation at a time) and lists.  Returns (codes as lists [gh][gw], the six arrays)."""
    _, H, W = xyz.shape
    gh, gw = -(-H // stride), -(-W // stride)
    k = [[bool(keep[gy * stride, gx * stride] != 0) for gx in range(gw)] for gy in range(gh)]
    z = [[float(xyz[2, gy * stride, gx * stride]) for gx in range(gw)] for gy in range(gh)]
    codes = [[0] * gw for _ in range(gh)]
    for cy in range(gh - 1):
        for cx in range(gw - 1):
            (ka, za), (kb, zb), (kc, zc), (kd, zd) = ((k[y][x], z[y][x]) for y, x in ((cy, cx), (cy, cx + 1), (cy + 1, cx), (cy + 1, cx + 1)))
            link = {e: loops_linked(*p, *q, cut) for e, (p, q) in dict(ab=((ka, za), (kb, zb)), ac=((ka, za), (kc, zc)), bd=((kb, zb), (kd, zd)),
                                                                     cd=((kc, zc), (kd, zd)), ad=((ka, za), (kd, zd)), bc=((kb, zb), (kc, zc))).items()}
            if ka and kd and (not (kb and kc) or abs(za - zd) <= abs(zb - zc)):
                t = (link["ac"] and link["cd"] and link["ad"], link["ad"] and link["bd"] and link["ab"], False, False)
            else:
                t = (False, False, link["ac"] and link["bc"] and link["ab"], link["bc"] and link["cd"] and link["bd"])
            codes[cy][cx] = sum(int(t[j]) << j for j in range(4))
    corners = {0: "acd", 1: "adb", 2: "acb", 3: "bcd"}
    tris = []      # triangles as node triples, in face order
    for cy in range(gh - 1):
        for cx in range(gw - 1):
            node = dict(a=(cy, cx), b=(cy, cx + 1), c=(cy + 1, cx), d=(cy + 1, cx + 1))
            for j in range(4):
                if codes[cy][cx] >> j & 1:
                    tris.append(tuple(node[c] for c in corners[j]))
    used = sorted({n for t in tris for n in t})
    place = {n: i for i, n in enumerate(used)}
    vert, nrm, rgb, uv, idx = [], [], [], [], []
    for gy, gx in used:
        v, u = gy * stride, gx * stride
        vert.append(xyz[:, v, u]), idx.append(v * W + u)
        nrm.append(normal[:, v, u] if normal is not None else np.zeros(3, f32))
        rgb.append(image[:, v, u] if image is not None else np.full(3, 255, np.uint8))
        uv.append((f32((float(u) + 0.5) / float(W)), f32((float(v) + 0.5) / float(H))))
    faces = [[place[n] for n in t] for t in tris]
    return codes, (np.array(vert, f32).reshape(-1, 3), np.array(nrm, f32).reshape(-1, 3), np.array(rgb, np.uint8).reshape(-1, 3),
                   np.array(uv, f32).reshape(-1, 2), np.array(idx, np.int32), np.array(faces, np.int32).reshape(-1, 3))


def host_codes(out, i, stride, cut):
    from genpercept_amd import mesh as ms
    return ms.cell_codes(*ms.grid_nodes(out["xyz"][i], out["keep"][i], stride), cut)


@pytest.mark.parametrize("space", ["depth", "disparity"])
@pytest.mark.parametrize("scene", SCENES, ids=lambda s: "%dx%d" % s)
def test_host_route_equals_plain_loops(scene, space):
    from genpercept_amd import geometry as gm
    from genpercept_amd import mesh as ms
    h, w = scene
    pred, mask, image, cam = random_case(np.random.RandomState(100 * h + w), h, w)
    faces = 0
    for stride, cut, use_mask, use_image in ((1, 0.05, False, True), (1, 0.2, True, False), (2, 0.05, True, True), (2, 0.2, False, False)):
        im, m = (image if use_image else None), (mask if use_mask else None)
        got = ms.depth_mesh(pred[None, None], cam, None if im is None else im[None], None if m is None else m[None], space, radius=1, stride=stride, cut=cut)
        geo = gm.depth_geometry(pred[None, None], cam, None, None if m is None else m[None], space, 1)
        assert all(same_bits(got[k], geo[k]) for k in PLANES)
        codes, want = loops_mesh(geo["xyz"][0], geo["normal"][0], geo["keep"][0], im, stride, cut)
        assert host_codes(got, 0, stride, cut).tolist() == codes
        for name, wv in zip(MESH, want):
            assert same_bits(got[name], wv), (scene, space, stride, cut, name)
        one = ms.mesh_from_planes(geo["xyz"][0], geo["normal"][0], geo["keep"][0], im, stride, cut)
        assert all(same_bits(a, b) for a, b in zip(one, want))
        assert ms.mesh_from_planes(geo["xyz"][0], None, geo["keep"][0], im, stride, cut)[1] is None
        for k, n in zip(OFFSETS, (len(want[0]), len(want[5]))):
            assert got[k].dtype == np.int64 and got[k].tolist() == [0, n]
        faces += len(want[5])
    assert faces > 0


# ---- the kernels' arithmetic on the CPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "mesh_check.cpp")


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: "%dx%d" % s)
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, scene, tmp_path):
    from genpercept_amd import mesh as ms
    h, w = scene
    pred, mask, image, cam = random_case(np.random.RandomState(7 * h + w), h, w)
    n_run = 0
    for space in ("depth", "disparity"):
        for stride, cut, use_mask, use_image, use_normal in ((1, 0.05, False, True, True), (1, 0.2, True, False, True), (2, 0.05, True, True, False),
                                                             (2, 0.2, False, False, True)):
            n_run += 1
            want = ms.depth_mesh(pred, cam, image if use_image else None, mask if use_mask else None, space, radius=1, stride=stride, cut=cut)
            xyz, normal, keep = (want[k][0] for k in PLANES)
            src, dst = str(tmp_path / f"in{n_run}.bin"), str(tmp_path / f"out{n_run}.bin")
            with open(src, "wb") as f:
                f.write(np.array([h, w, stride, use_normal, use_image, 0], np.int32).tobytes() + np.array([cut], f64).tobytes() + xyz.tobytes()
                        + (normal.tobytes() if use_normal else b"") + keep.tobytes() + (image.tobytes() if use_image else b""))
            raw = ps.run_check(check_exe, src, dst)[1]
            codes = host_codes(want, 0, stride, cut)
            assert same_bits(np.frombuffer(raw[:codes.size], np.uint8).reshape(codes.shape), codes), (scene, space, stride, cut)
            pos = codes.size
            n, m = (int(v) for v in np.frombuffer(raw[pos:pos + 16], np.int64))
            pos += 16
            assert [n, m] == [want["vertex_offsets"][1], want["face_offsets"][1]]
            for name, dt, width in (("vertices", f32, 3), ("vertex_normals", f32, 3), ("vertex_rgb", np.uint8, 3), ("vertex_uv", f32, 2),
                                    ("vertex_index", np.int32, 1), ("faces", np.int32, 3)):
                if name == "vertex_normals" and not use_normal:
                    continue
                count = (m if name == "faces" else n) * width
                got = np.frombuffer(raw[pos:pos + count * np.dtype(dt).itemsize], dt)
                pos += got.nbytes
                assert same_bits(got.reshape(want[name].shape), want[name]), (scene, space, stride, cut, name)
            assert pos == len(raw)


# ---- what the definition is for ----------------------------------------------------------------------------------------------------------------------
def test_the_coverage_scene_holds_every_code_and_an_unused_kept_node():
    """random_case(RandomState(940), 17, 23) with its mask, depth space, radius 1, stride 1, cut 0.05: 273 kept nodes of which 243 are vertices,
    267 triangles, and every code of 1, 2, 3, 4, 8, 12 occurs.  The device test of this size runs the same scene: the condition is asserted
    so that a changed scene cannot hollow it out."""
    from genpercept_amd import mesh as ms
    pred, mask, image, cam = random_case(np.random.RandomState(940), 17, 23)
    got = ms.depth_mesh(pred, cam, image, mask, "depth", radius=1, stride=1, cut=0.05)
    codes = host_codes(got, 0, 1, 0.05)
    assert set(codes.ravel().tolist()) == {0, 1, 2, 3, 4, 8, 12}
    kept = int((got["keep"] != 0).sum())
    print(f"coverage scene: {kept} kept nodes, {len(got['vertices'])} vertices, {len(got['faces'])} faces")
    assert (kept, len(got["vertices"]), len(got["faces"])) == (273, 243, 267)
    assert len(got["vertices"]) < kept and set(got["vertex_index"].tolist()) < set(np.flatnonzero(got["keep"][0]).tolist())


def flat_planes(z):
    """(xyz float32 [3, H, W], normal, keep) of a depth plane z [H, W] (NaN: not kept) under a camera with f = 20 and its principal point at the centre"""
    h, w = z.shape
    v, u = np.mgrid[0:h, 0:w].astype(f64)
    xyz = np.stack([(u - (w - 1) / 2.0) / 20.0 * z, (v - (h - 1) / 2.0) / 20.0 * z, z]).astype(f32)
    normal = np.zeros((3, h, w), f32)
    normal[2] = -1.0
    return xyz, normal, (~np.isnan(z)).astype(np.uint8)


def test_a_fronto_parallel_plane_is_fully_meshed():
    from genpercept_amd import mesh as ms
    for h, w, stride in ((7, 9, 1), (10, 13, 3), (6, 6, 2)):
        xyz, normal, keep = flat_planes(np.full((h, w), 1.5))
        gh, gw = -(-h // stride), -(-w // stride)
        codes = ms.cell_codes(*ms.grid_nodes(xyz, keep, stride), 0.05)
        assert (codes[:-1, :-1] == 3).all() and not codes[-1].any() and not codes[:, -1].any()
        vert, nrm, rgb, uv, idx, faces = ms.mesh_from_planes(xyz, normal, keep, None, stride, 0.05)
        assert len(faces) == 2 * (gh - 1) * (gw - 1) and len(vert) == gh * gw and (rgb == 255).all()
        assert idx.tolist() == [gy * stride * w + gx * stride for gy in range(gh) for gx in range(gw)]
        assert same_bits(uv, np.array([[f32((gx * stride + 0.5) / w), f32((gy * stride + 0.5) / h)] for gy in range(gh) for gx in range(gw)], f32))
        assert faces[:2].tolist() == [[0, gw, gw + 1], [0, gw + 1, 1]]


def test_no_face_crosses_a_depth_step_and_one_near_corner_leaves_the_far_triangle():
    from genpercept_amd import mesh as ms
    h, w = 8, 10
    z = np.full((h, w), 2.0)
    z[:, :5] = 1.0                                                      # near on the left: a step of 100 % of the nearer depth
    xyz, normal, keep = flat_planes(z)
    for cut in (0.05, 0.2, 0.99):
        vert, _, _, _, idx, faces = ms.mesh_from_planes(xyz, normal, keep, None, 1, cut)
        side = (idx % w) < 5
        assert len(faces) == 2 * (h - 1) * (w - 2) and len(vert) == h * w
        assert (side[faces].all(1) | (~side[faces]).all(1)).all()
    assert len(ms.mesh_from_planes(xyz, normal, keep, None, 1, 1.0)[5]) == 2 * (h - 1) * (w - 1)   # |1 - 2| <= 1.0 * 1: the step is joined
    # one cell, one near corner: exactly the far-side triangle, on the diagonal that does not touch the near corner
    want = dict(a=(8, "bcd"), b=(1, "acd"), c=(2, "adb"), d=(4, "acb"))
    place = dict(a=0, b=1, c=2, d=3)
    for corner, (code, tri) in want.items():
        z = np.full((2, 2), 2.0)
        z[place[corner] // 2, place[corner] % 2] = 1.0
        xyz, normal, keep = flat_planes(z)
        assert ms.cell_codes(*ms.grid_nodes(xyz, keep, 1), 0.05).tolist() == [[code, 0], [0, 0]]
        vert, _, _, _, idx, faces = ms.mesh_from_planes(xyz, normal, keep, None, 1, 0.05)
        far = [place[c] for c in tri]
        assert idx.tolist() == sorted(far) and faces.tolist() == [[sorted(far).index(p) for p in far]], corner
        # the same corner not kept at all: the same triangle (three kept corners leave at most that one)
        keep[place[corner] // 2, place[corner] % 2] = 0
        assert ms.mesh_from_planes(xyz, normal, keep, None, 1, 0.05)[5].tolist() == faces.tolist()
    # a tie goes to a-d; a NaN depth at a kept node fails every link it is part of
    xyz, normal, keep = flat_planes(np.array([[1.0, 1.01], [1.01, 1.0]]))
    assert ms.cell_codes(*ms.grid_nodes(xyz, keep, 1), 0.05)[0, 0] == 3
    xyz[2, 0, 0] = np.nan
    assert ms.cell_codes(*ms.grid_nodes(xyz, keep, 1), 0.05)[0, 0] == 8


def batch_of_three(seed=11, h=21, w=30, middle_empty=True):
    rng = np.random.RandomState(seed)
    per = [random_case(rng, h, w) for _ in range(3)]
    pred, mask, image, cams = (np.stack([p[k] for p in per]) for k in range(4))
    if middle_empty:
        mask[1] = 0
    return pred[:, None], mask, image, cams


def test_faces_look_at_the_camera_and_the_surface_is_an_oriented_manifold():
    from genpercept_amd import mesh as ms
    pred, mask, image, cams = batch_of_three(middle_empty=False)
    for stride, cut in ((1, 0.05), (1, 0.2), (2, 0.2)):
        got = ms.depth_mesh(pred, cams, image, mask, "depth", radius=1, stride=stride, cut=cut)
        vo, fo = got["vertex_offsets"], got["face_offsets"]
        for i in range(3):
            p = got["vertices"][vo[i]:vo[i + 1]].astype(f64)
            faces = got["faces"][fo[i]:fo[i + 1]]
            assert len(faces) > 0
            v0, v1, v2 = (p[faces[:, k]] for k in range(3))
            assert ((np.cross(v1 - v0, v2 - v0) * v0).sum(1) < 0).all()
            directed = {}
            for t in faces.tolist():
                for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                    directed[e] = directed.get(e, 0) + 1
            assert all(n == 1 for n in directed.values())              # no directed edge twice: at most two faces per edge, opposite ways
            assert set(np.unique(faces).tolist()) == set(range(len(p)))  # every vertex is used


def test_indices_offsets_and_an_empty_image_in_the_middle():
    from genpercept_amd import mesh as ms
    pred, mask, image, cams = batch_of_three()
    h, w = pred.shape[-2:]
    for stride in (1, 2, 3):
        got = ms.depth_mesh(pred, cams, image, mask, "depth", radius=1, stride=stride, cut=0.2)
        vo, fo = got["vertex_offsets"], got["face_offsets"]
        for off, n in ((vo, len(got["vertices"])), (fo, len(got["faces"]))):
            assert off.dtype == np.int64 and off.shape == (4,) and off[0] == 0 and off[1] == off[2] and off[3] == n > 0 and (np.diff(off) >= 0).all()
        assert all(len(got[k]) == vo[3] for k in MESH[:5]) and got["faces"].dtype == np.int32 and got["vertex_index"].dtype == np.int32
        for i in range(3):
            idx, faces = got["vertex_index"][vo[i]:vo[i + 1]], got["faces"][fo[i]:fo[i + 1]]
            assert (np.diff(idx) > 0).all() and ((idx % w) % stride == 0).all() and ((idx // w) % stride == 0).all()
            assert len(faces) == 0 or (faces.min() >= 0 and faces.max() < len(idx))
            assert (got["keep"][i].ravel()[idx] != 0).all()
            assert same_bits(got["vertices"][vo[i]:vo[i + 1]], got["xyz"][i].reshape(3, -1)[:, idx].T)
            assert same_bits(got["vertex_normals"][vo[i]:vo[i + 1]], got["normal"][i].reshape(3, -1)[:, idx].T)
            assert same_bits(got["vertex_rgb"][vo[i]:vo[i + 1]], image[i].reshape(3, -1)[:, idx].T)
            one = ms.depth_mesh(pred[i], cams[i], image[i], mask[i], "depth", radius=1, stride=stride, cut=0.2)
            assert all(same_bits(one[k], got[k][(fo if k == "faces" else vo)[i]:(fo if k == "faces" else vo)[i + 1]]) for k in MESH)
        assert (ms.depth_mesh(pred, cams, None, mask, radius=1, stride=stride, cut=0.2)["vertex_rgb"] == 255).all()


def test_degenerate_grids_give_empty_meshes():
    from genpercept_amd import mesh as ms
    for h, w, stride in ((1, 70, 1), (7, 1, 1), (5, 9, 64), (5, 9, 9), (6, 40, 6), (40, 3, 3)):
        pred = np.full((2, 1, h, w), 0.5, f32)
        got = ms.depth_mesh(pred, stride=stride, radius=1, min_count=3)
        assert got["vertex_offsets"].tolist() == [0, 0, 0] and got["face_offsets"].tolist() == [0, 0, 0]
        for k, shape, dt in zip(MESH, ((0, 3), (0, 3), (0, 3), (0, 2), (0,), (0, 3)), (f32, f32, np.uint8, f32, np.int32, np.int32)):
            assert got[k].shape == shape and got[k].dtype == dt, k


# ---- the writers ---------------------------------------------------------------------------------------------------------------------------------------
COMPONENT = {5126: ("<f4", 4), 5125: ("<u4", 4), 5121: ("u1", 1)}
WIDTH = dict(SCALAR=1, VEC2=2, VEC3=3, VEC4=4)


def parse_glb(path):
    """A .glb file by the container's rules: (the JSON, a function accessor index -> array, a function bufferView index -> bytes)."""
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack("<4sII", raw[:12])
    assert magic == b"glTF" and version == 2 and total == len(raw) == os.path.getsize(path)
    n_json, kind = struct.unpack("<I4s", raw[12:20])
    assert kind == b"JSON" and n_json % 4 == 0
    doc = json.loads(raw[20:20 + n_json].decode("ascii"))
    assert raw[20:20 + n_json].rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode("ascii")   # padded with spaces only
    pos, body = 20 + n_json, b""
    if pos < len(raw):
        n_bin, kind = struct.unpack("<I4s", raw[pos:pos + 8])
        assert kind == b"BIN\0" and n_bin % 4 == 0 and pos % 4 == 0 and pos + 8 + n_bin == len(raw)     # two chunks, in order, nothing after
        body = raw[pos + 8:]
        assert doc["buffers"] == [dict(byteLength=n_bin)]
    else:
        assert "buffers" not in doc and "bufferViews" not in doc
    assert doc["asset"]["version"] == "2.0"

    def view(i):
        bv = doc["bufferViews"][i]
        assert bv["buffer"] == 0 and bv["byteOffset"] % 4 == 0 and bv["byteOffset"] + bv["byteLength"] <= len(body)
        return body[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]]

    def accessor(i):
        a = doc["accessors"][i]
        dt, size = COMPONENT[a["componentType"]]
        arr = np.frombuffer(view(a["bufferView"]), dt)
        assert arr.size == a["count"] * WIDTH[a["type"]]
        return arr.reshape(a["count"], WIDTH[a["type"]]) if a["type"] != "SCALAR" else arr

    return doc, accessor, view


def test_write_glb(tmp_path):
    from PIL import Image
    from genpercept_amd import mesh as ms
    pred, mask, image, cam = random_case(np.random.RandomState(940), 17, 23)
    got = ms.depth_mesh(pred, cam, image, mask, "depth", radius=1, cut=0.05)
    vert, nrm, rgb, uv, faces = (got[k] for k in ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "faces"))
    n, m = len(vert), len(faces)
    flipped = np.stack([vert[:, 0], -vert[:, 1], -vert[:, 2]], 1)
    for textured, with_normals in ((True, True), (False, True), (False, False)):
        path = str(tmp_path / f"m{textured}{with_normals}.glb")
        ms.write_glb(path, vert, nrm if with_normals else None, uv, faces, image=image if textured else None, rgb=None if textured else rgb)
        doc, accessor, view = parse_glb(path)
        assert doc["scene"] == 0 and doc["scenes"] == [dict(nodes=[0])] and doc["nodes"] == [dict(mesh=0)] and len(doc["meshes"]) == 1
        (prim,) = doc["meshes"][0]["primitives"]
        att = prim["attributes"]
        assert sorted(att) == sorted(["POSITION", "TEXCOORD_0"] + (["NORMAL"] if with_normals else []) + ([] if textured else ["COLOR_0"]))
        pos_acc = doc["accessors"][att["POSITION"]]
        assert pos_acc["count"] == n and pos_acc["type"] == "VEC3" and pos_acc["componentType"] == 5126
        assert same_bits(accessor(att["POSITION"]), flipped, f32)                                    # (x, -y, -z) bit for bit
        assert pos_acc["min"] == [float(v) for v in flipped.min(0)] and pos_acc["max"] == [float(v) for v in flipped.max(0)]
        assert same_bits(accessor(att["TEXCOORD_0"]), uv, f32) and doc["accessors"][att["TEXCOORD_0"]]["count"] == n
        if with_normals:
            assert same_bits(accessor(att["NORMAL"]), np.stack([nrm[:, 0], -nrm[:, 1], -nrm[:, 2]], 1), f32)
        ind = doc["accessors"][prim["indices"]]
        assert ind["count"] == 3 * m and ind["componentType"] == 5125 and ind["type"] == "SCALAR"
        index = accessor(prim["indices"])
        assert index.max() < n and np.array_equal(index.reshape(m, 3), faces)
        (material,) = doc["materials"]
        pbr = material["pbrMetallicRoughness"]
        assert material["doubleSided"] is True and pbr["metallicFactor"] == 0.0 and pbr["roughnessFactor"] == 1.0 and prim["material"] == 0
        if textured:
            assert pbr["baseColorTexture"] == dict(index=0) and doc["textures"] == [dict(sampler=0, source=0)] and doc["images"][0]["mimeType"] == "image/png"
            png = np.asarray(Image.open(io.BytesIO(view(doc["images"][0]["bufferView"]))))
            assert png.dtype == np.uint8 and np.array_equal(png, image.transpose(1, 2, 0))
        else:
            col = doc["accessors"][att["COLOR_0"]]
            assert "baseColorTexture" not in pbr and col["normalized"] is True and col["type"] == "VEC4"
            assert np.array_equal(accessor(att["COLOR_0"]), np.concatenate([rgb, np.full((n, 1), 255, np.uint8)], 1))
    # no faces: a valid file whose scene has no mesh
    path = str(tmp_path / "empty.glb")
    ms.write_glb(path, vert[:0], nrm[:0], uv[:0], faces[:0], image=image)
    doc, _, _ = parse_glb(path)
    assert doc["scene"] == 0 and doc["scenes"] == [{}] and "meshes" not in doc and "nodes" not in doc and "accessors" not in doc
    for bad in (dict(uv=uv[:-1]), dict(normals=nrm[:-1]), dict(faces=faces + n), dict(faces=faces.astype(f32)), dict(image=image[0]), dict(rgb=rgb[:-1])):
        with pytest.raises(ValueError):
            ms.write_glb(path, **dict(dict(vertices=vert, normals=nrm, uv=uv, faces=faces), **bad))


def read_mesh_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    n, m = int(lines[2].split()[-1]), int(lines[12].split()[-1])
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2] == f"element vertex {n}" and lines[12] == f"element face {m}"
    assert lines[3:12] == [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {k}" for k in ("red", "green", "blue")]
    assert lines[13:] == ["property list uchar int vertex_indices"] and len(body) == 27 * n + 13 * m
    rec = np.frombuffer(body[:27 * n], np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    face = np.frombuffer(body[27 * n:], np.dtype([("k", "u1"), ("v", "<i4", 3)]))
    assert (face["k"] == 3).all()
    return rec["p"], rec["n"], rec["c"], face["v"]


def test_write_mesh_ply(tmp_path):
    from genpercept_amd import mesh as ms
    pred, mask, image, cam = random_case(np.random.RandomState(940), 17, 23)
    got = ms.depth_mesh(pred, cam, image, mask, "depth", radius=1, cut=0.05)
    path = str(tmp_path / "m.ply")
    for sl in (slice(None), slice(0, 0)):
        faces = got["faces"][sl]
        n = len(got["vertices"]) if len(faces) else 0
        ms.write_mesh_ply(path, got["vertices"][:n], got["vertex_normals"][:n], got["vertex_rgb"][:n], faces)
        p, nr, c, fv = read_mesh_ply(path)
        assert same_bits(p, got["vertices"][:n]) and same_bits(nr, got["vertex_normals"][:n]) and same_bits(c, got["vertex_rgb"][:n])
        assert same_bits(np.ascontiguousarray(fv), faces, np.int32)
    with pytest.raises(ValueError):
        ms.write_mesh_ply(path, got["vertices"], got["vertex_normals"], got["vertex_rgb"][:-1], got["faces"])
    with pytest.raises(ValueError):
        ms.write_mesh_ply(path, got["vertices"][:5], got["vertex_normals"][:5], got["vertex_rgb"][:5], got["faces"])


def test_options_and_shapes_are_checked():
    import math
    from genpercept_amd import mesh as ms
    cos85 = math.cos(math.radians(85.0))
    assert ms.mesh_options(True) == dict(radius=2, tau=0.05, min_count=5, min_cos=cos85, stride=1, cut=0.05) and ms.CUT_DEFAULT == 0.05
    assert ms.mesh_options(dict(radius=8, stride=64, cut=1.0)) == dict(radius=8, tau=0.05, min_count=17, min_cos=cos85, stride=64, cut=1.0)
    assert ms.check_mesh_options(cut=1) == ms.mesh_options(dict(cut=1.0))
    for bad in (False, None, 1, "yes", dict(r=2), dict(edge=0.1), dict(radius=0), dict(radius=9), dict(tau=0.0), dict(min_count=2), dict(min_cos=1.0),
                dict(stride=0), dict(stride=65), dict(stride=2.0), dict(cut=0), dict(cut=0.0), dict(cut=-0.1), dict(cut=1.0000001), dict(cut=float("nan")),
                dict(cut=True), dict(cut="0.05"), dict(cut=None)):
        with pytest.raises(ValueError):
            ms.mesh_options(bad)
    pred = np.broadcast_to((0.2 + 0.02 * np.arange(6)[:, None] + 0.01 * np.arange(7)[None, :]).astype(f32), (2, 1, 6, 7))
    got = ms.depth_mesh(pred, radius=1, cut=1.0)
    assert sorted(got) == sorted(PLANES + MESH + OFFSETS) and got["face_offsets"][-1] > 0
    for bad in (dict(cut=0.0), dict(cut=float("nan")), dict(stride=0), dict(stride=65), dict(radius=9), dict(space="metric"), dict(cameras=np.ones(7)),
                dict(image=np.zeros((2, 3, 6, 6), np.uint8)), dict(mask=np.ones((2, 7, 6), bool))):
        with pytest.raises(ValueError):
            ms.depth_mesh(pred, **bad)
    xyz, normal, keep = got["xyz"][0], got["normal"][0], got["keep"][0]
    for bad in (dict(xyz=xyz.astype(f64)), dict(xyz=xyz[:2]), dict(keep=keep[:, :5]), dict(normal=normal[:, :5]), dict(image=np.zeros((3, 6, 7), f32)),
                dict(stride=0), dict(stride=65), dict(stride=True), dict(cut=0.0), dict(cut=float("nan")), dict(cut=2.0)):
        with pytest.raises(ValueError):
            ms.mesh_from_planes(**dict(dict(xyz=xyz, normal=normal, keep=keep, image=None, stride=1, cut=0.05), **bad))


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine, infer_eval, pipeline
    hdr, math_h = ps.assert_entries_bound(NAMES, "depth_mesh.hip", "depth_mesh_math.h")
    args = engine.SYMBOLS["gp_depth_mesh"][1]
    assert len(args) == 20 and args[8] is C.c_double and engine.SYMBOLS["gp_depth_mesh_workspace"] == (C.c_longlong, [C.c_int] * 4)
    assert callable(engine.depth_mesh) and callable(infer_eval.run_meshes)
    assert callable(pipeline.GenPerceptPipeline.mesh_batch_device) and callable(pipeline.GenPerceptPipeline.mesh)
    assert "hip_runtime" not in math_h and "point to the camera" in hdr
    # one copy of the grid and the scan: both ops take them from the shared header
    csrc = os.path.join(ps.ROOT, "genpercept_amd", "csrc")
    for src in ("depth_geometry.hip", "depth_mesh.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "depth_grid.h"' in text and "__shfl_up" not in text and "struct DgGrid" not in text and "atomicAdd" not in text
    assert open(os.path.join(csrc, "depth_mesh.hip")).read().count("hipLaunchKernelGGL(") <= 5


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 64, 64, 1), (65536, 8, 8, 1), (1, 0, 64, 1), (1, 64, 16385, 1), (1, 64, 64, 0), (1, 64, 64, 65), (8, 16384, 16384, 1), (-1, 64, 64, 1),
                    (4, 16384, 16384, 1), (7, 16384, 16384, 1)):                            # the last two: B gh gw >= 2^30
            assert lib.gp_depth_mesh_workspace(*bad) == 0, bad
        for h, w, stride in ((17, 23, 1), (33, 200, 3), (768, 768, 1), (2048, 3072, 2), (16384, 16384, 64), (1, 70, 1), (5, 9, 64)):
            one = lib.gp_depth_mesh_workspace(1, h, w, stride)
            assert one > 0 and one % 8 == 0 and one >= (-(-h // stride)) * (-(-w // stride))
            for b in (2, 7):
                assert lib.gp_depth_mesh_workspace(b, h, w, stride) == b * one
        assert lib.gp_depth_mesh_workspace(3, 16384, 16384, 1) > 0 and lib.gp_depth_mesh_workspace(7, 16384, 16384, 2) > 0


def mesh_args(lib, b, h, w, stride=1, **ptrs):
    """A valid argument set of gp_depth_mesh for these sizes (pointers as given, small integers by default)."""
    ok = dict(xyz=0x1000, normal=0x2000, keep=0x3001, image=0x4003, B=b, H=h, W=w, stride=stride, cut=0.05, vertices=0x5000, vertex_normals=0x6000,
              vertex_rgb=0x7001, vertex_uv=0x8000, vertex_index=0x9000, faces=0xA000, vertex_offsets=0xB000, face_offsets=0xB800, ws=0xC000,
              nbytes=int(lib.gp_depth_mesh_workspace(b, h, w, stride)))
    ok.update(ptrs)
    return ok


def invalid_cases(ok):
    """The argument sets gp_depth_mesh refuses, as changes to a valid set `ok`."""
    huge = 1 << 62
    return [dict(xyz=None), dict(keep=None), dict(vertex_offsets=None), dict(face_offsets=None), dict(ws=None),
            dict(B=0), dict(B=-1), dict(B=65536, nbytes=huge), dict(H=0), dict(W=-5), dict(H=16385, nbytes=huge), dict(W=16385, nbytes=huge),
            dict(B=8, H=16384, W=16384, nbytes=huge),                                            # B H W = 2^31
            dict(B=4, H=16384, W=16384, nbytes=huge),                                            # B gh gw = 2^30
            dict(stride=0), dict(stride=65), dict(stride=-1), dict(cut=0.0), dict(cut=-0.5), dict(cut=1.0000001), dict(cut=float("nan")),
            dict(cut=float("inf")), dict(normal=None),                                           # vertex_normals without normal
            dict(xyz=ok["xyz"] + 2), dict(xyz=ok["xyz"] + 1), dict(normal=ok["normal"] + 2), dict(vertices=ok["vertices"] + 2),
            dict(vertex_normals=ok["vertex_normals"] + 1), dict(vertex_uv=ok["vertex_uv"] + 2), dict(vertex_index=ok["vertex_index"] + 3),
            dict(faces=ok["faces"] + 2), dict(vertex_offsets=ok["vertex_offsets"] + 4), dict(face_offsets=ok["face_offsets"] + 4),
            dict(face_offsets=ok["face_offsets"] + 1), dict(ws=ok["ws"] + 4), dict(ws=ok["ws"] + 1),
            dict(nbytes=ok["nbytes"] - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=ok["nbytes"] // 2)]


def call_mesh(lib, a):
    return lib.gp_depth_mesh(a["xyz"], a["normal"], a["keep"], a["image"], a["B"], a["H"], a["W"], a["stride"], a["cut"], a["vertices"], a["vertex_normals"],
                             a["vertex_rgb"], a["vertex_uv"], a["vertex_index"], a["faces"], a["vertex_offsets"], a["face_offsets"], a["ws"], a["nbytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        ok = mesh_args(lib, 2, 40, 70)
        assert ok["nbytes"] > 0
        ps.assert_all_refused(call_mesh, lib, ok, invalid_cases(ok))
