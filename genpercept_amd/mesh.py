"""Triangle meshes from the point map of a depth prediction, the host route (numpy, no torch): the nodes of the stride grid are joined to
their neighbours wherever both are kept and their depths are close, so the surface is cut at depth edges and has no "rubber sheet" across
them; the nodes that a triangle uses become vertices, the triangles faces; `write_glb` and `write_mesh_ply` save one image's mesh.  This
file is the specification in executable form; csrc/depth_mesh.hip (gp_depth_mesh) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the per-cell arithmetic once more in csrc/depth_mesh_math.h)
  Per image: xyz float32 [3, H, W] as `geometry.depth_geometry` writes them; normal float32 [3, H, W], optional; keep uint8 [H, W]; image uint8
    [3, H, W], optional.  Per call: stride in 1 .. 64; cut, float64 in (0, 1] (a NaN is refused).  1 <= H, W <= 16384, 1 <= B <= 65535,
    B * H * W < 2^31 and B * gh * gw < 2^30, so the triangle count stays below 2^31.
  Grid: gh = ceil(H / stride), gw = ceil(W / stride); node (gy, gx) is the pixel (v, u) = (gy * stride, gx * stride); its k is keep != 0, its z
    is plane 2 of xyz, promoted to float64.
  Link: two nodes p, q are linked iff both are kept and |z_p - z_q| <= cut * min(z_p, z_q): float64, one subtraction, fabs, one min, one product,
    one compare, no fused multiply-add.  A NaN fails the test.
  Cell (cy, cx), cy < gh - 1 and cx < gw - 1: corners a = (cy, cx), b = (cy, cx + 1), c = (cy + 1, cx), d = (cy + 1, cx + 1).  Candidate
    triangles T0 = (a, c, d), T1 = (a, d, b) on diagonal a-d; T2 = (a, c, b), T3 = (b, c, d) on diagonal b-c.  A triangle is sound iff each of its
    three edges is linked.  The cell uses a-d iff k_a and k_d hold and also one of these: k_b and k_c do not both hold, or
    |z_a - z_d| <= |z_b - z_c| (a tie goes to a-d); otherwise b-c.  It emits the sound triangles of its diagonal and nothing from the other;
    there is no fallback.  So one foreground corner over a background leaves the one background triangle.  The cell's code is
    T0 | T1 << 1 | T2 << 2 | T3 << 3: 0, 1, 2, 3, 4, 8 or 12.
  Winding: the corner orders make (v1 - v0) x (v2 - v0) point to the camera: its dot product with v0 is negative (camera at the origin, x
    right, y down, z forward).
  Vertices: a node is a vertex iff an emitted triangle uses it; kept pixels that end up in no triangle are not exported.  Row-major node
    order, image after image: vertices float32 [n, 3] from xyz, vertex_normals float32 [n, 3] from normal, vertex_rgb uint8 [n, 3] (255 without
    an image), vertex_uv float32 [n, 2] = ((u + 0.5) / W, (v + 0.5) / H) in float64, each rounded once, vertex_index int32 [n] = v * W + u.
  Faces: cells in row-major order, image after image; within a cell T0 before T1, or T2 before T3.  faces int32 [m, 3], indices local to the
    image (the global vertex index minus vertex_offsets[b]): each image's mesh stands alone.
  Offsets: vertex_offsets and face_offsets int64 [B + 1].

The default cut = 0.05 (`CUT_DEFAULT`) is a CONVENTION, not a measurement: neighbours whose depths differ by more than 5 % of the nearer one
are not joined.  It equals the default tau of the plane fit, so a surface that one window fits is one the mesh joins.
"""
from __future__ import annotations

import json
import struct
from typing import Dict, Optional

import numpy as np

from . import geometry
from .post_common import MAX_DIM, is_int, options_from

CUT_DEFAULT = 0.05
DEFAULTS = dict(geometry.DEFAULTS, cut=CUT_DEFAULT)
MAX_NODES = 2 ** 30
MESH_ARRAYS = ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "vertex_index", "faces")
f32, f64 = np.float32, np.float64


def check_cut(cut) -> float:
    if isinstance(cut, bool) or not isinstance(cut, (int, float, np.integer, np.floating)) or not (0.0 < float(cut) <= 1.0):
        raise ValueError(f"cut is in (0, 1], got {cut!r}")
    return float(cut)


def check_mesh_options(radius=2, tau=0.05, min_count=None, min_cos=None, stride=1, cut=CUT_DEFAULT) -> Dict:
    """The ranges of the definition and of `geometry.check_options` (ValueError outside them), with the defaults filled in."""
    opts = dict(zip(geometry.DEFAULTS, geometry.check_options(radius, tau, min_count, min_cos, stride)))
    opts["cut"] = check_cut(cut)
    return opts


def mesh_options(mesh) -> Dict:
    """The `mesh` argument of the pipeline entries -- True or a dict with the keys radius, tau, min_count, min_cos, stride, cut -- as the
    checked options of `depth_mesh`."""
    return options_from(mesh, DEFAULTS, "mesh", lambda o: check_mesh_options(**o))


def grid_nodes(xyz, keep, stride: int):
    """(z float64 [gh, gw], k bool [gh, gw]) of the stride grid of one image."""
    return np.asarray(xyz)[2, ::stride, ::stride].astype(f64), np.asarray(keep)[::stride, ::stride] != 0


def _linked(zp, kp, zq, kq, cut: float):
    with np.errstate(all="ignore"):
        return kp & kq & (np.abs(zp - zq) <= f64(cut) * np.minimum(zp, zq))    # (False for a NaN on either side)


def cell_codes(z, k, cut: float) -> np.ndarray:
    """The four-bit codes of the cells as a node-shaped plane uint8 [gh, gw], 0 in the last row and column."""
    gh, gw = z.shape
    codes = np.zeros((gh, gw), np.uint8)
    if gh < 2 or gw < 2:
        return codes
    (za, ka), (zb, kb), (zc, kc), (zd, kd) = ((z[sy, sx], k[sy, sx]) for sy, sx in ((slice(0, -1), slice(0, -1)), (slice(0, -1), slice(1, None)),
                                                                                   (slice(1, None), slice(0, -1)), (slice(1, None), slice(1, None))))
    ab, ac, bd, cd = _linked(za, ka, zb, kb, cut), _linked(za, ka, zc, kc, cut), _linked(zb, kb, zd, kd, cut), _linked(zc, kc, zd, kd, cut)
    ad, bc = _linked(za, ka, zd, kd, cut), _linked(zb, kb, zc, kc, cut)
    with np.errstate(all="ignore"):
        use_ad = ka & kd & (~(kb & kc) | (np.abs(za - zd) <= np.abs(zb - zc)))
    t0, t1 = use_ad & ad & ac & cd, use_ad & ad & bd & ab
    t2, t3 = ~use_ad & bc & ac & ab, ~use_ad & bc & cd & bd
    codes[:-1, :-1] = t0 | (t1.astype(np.uint8) << 1) | (t2.astype(np.uint8) << 2) | (t3.astype(np.uint8) << 3)
    return codes


def used_nodes(codes: np.ndarray) -> np.ndarray:
    """bool [gh, gw]: the nodes that a triangle of one of their four cells uses (corner a of the cell at the node, b of the cell to its left,
    c of the cell above, d of the cell above left)."""
    used = (codes & 7) != 0
    used[:, 1:] |= (codes[:, :-1] & 14) != 0
    used[1:, :] |= (codes[:-1, :] & 13) != 0
    used[1:, 1:] |= (codes[:-1, :-1] & 11) != 0
    return used


def mesh_from_planes(xyz, normal, keep, image, stride: int = 1, cut: float = CUT_DEFAULT):
    """One image by the definition above: (vertices float32 [n, 3], vertex_normals float32 [n, 3] or None without `normal`, vertex_rgb uint8
    [n, 3], vertex_uv float32 [n, 2], vertex_index int32 [n], faces int32 [m, 3])."""
    xyz, keep = np.asarray(xyz), np.asarray(keep)
    if not is_int(stride) or not 1 <= stride <= geometry.MAX_STRIDE:
        raise ValueError(f"stride is an integer in 1 .. {geometry.MAX_STRIDE}, got {stride!r}")
    cut = check_cut(cut)
    if xyz.ndim != 3 or xyz.shape[0] != 3 or xyz.dtype != f32 or keep.shape != xyz.shape[1:]:
        raise ValueError(f"xyz float32 [3, H, W] and keep [H, W], got {xyz.dtype} {xyz.shape} and {keep.shape}")
    H, W = keep.shape
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"sides in 1 .. {MAX_DIM}, got {(H, W)}")
    for name, plane, dt in (("normal", normal, f32), ("image", image, np.uint8)):
        if plane is not None and (np.shape(plane) != (3, H, W) or np.asarray(plane).dtype != dt):
            raise ValueError(f"{name}: {np.dtype(dt)} {(3, H, W)}, got {np.asarray(plane).dtype} {np.shape(plane)}")
    z, k = grid_nodes(xyz, keep, stride)
    gh, gw = z.shape
    codes = cell_codes(z, k, cut)
    used = used_nodes(codes)
    gy, gx = np.nonzero(used)
    v, u = gy * stride, gx * stride
    idx = v * W + u
    vertices = np.ascontiguousarray(xyz.reshape(3, H * W)[:, idx].T)
    normals = None if normal is None else np.ascontiguousarray(np.asarray(normal).reshape(3, H * W)[:, idx].T)
    rgb = np.full((len(idx), 3), 255, np.uint8) if image is None else np.ascontiguousarray(np.asarray(image).reshape(3, H * W)[:, idx].T)
    uv = np.stack([((u.astype(f64) + f64(0.5)) / f64(W)).astype(f32), ((v.astype(f64) + f64(0.5)) / f64(H)).astype(f32)], 1).reshape(-1, 2)
    place = (np.cumsum(used.ravel()) - 1).reshape(gh, gw)           # a used node's vertex index
    if gh < 2 or gw < 2:
        faces = np.zeros((0, 3), np.int32)
    else:
        a, b, c, d = place[:-1, :-1], place[:-1, 1:], place[1:, :-1], place[1:, 1:]
        code = codes[:-1, :-1]
        first = np.where(((code & 1) != 0)[..., None], np.stack([a, c, d], -1), np.stack([a, c, b], -1))
        second = np.where(((code & 2) != 0)[..., None], np.stack([a, d, b], -1), np.stack([b, c, d], -1))
        both = np.stack([first, second], 2)                          # [gh - 1, gw - 1, 2, 3]
        has = np.stack([(code & 5) != 0, (code & 10) != 0], 2)
        faces = np.ascontiguousarray(both[has].astype(np.int32)).reshape(-1, 3)
    return vertices, normals, rgb, np.ascontiguousarray(uv), idx.astype(np.int32), faces


def depth_mesh(pred, cameras=None, image=None, mask=None, space: str = "depth", radius=2, tau=0.05, min_count=None, min_cos=None, stride=1,
               cut=CUT_DEFAULT) -> Dict:
    """A batch: `geometry.depth_geometry` of the same arguments, then the mesh of every image by the definition above.  Returns a dict with
    that function's planes xyz float32 [B, 3, H, W], normal float32 [B, 3, H, W], keep uint8 [B, H, W] and vertices, vertex_normals float32 [n, 3],
    vertex_rgb uint8 [n, 3], vertex_uv float32 [n, 2], vertex_index int32 [n], faces int32 [m, 3] (indices local to the image), vertex_offsets
    and face_offsets int64 [B + 1] (image k owns the vertices vertex_offsets[k] .. vertex_offsets[k + 1] and the faces likewise)."""
    opts = check_mesh_options(radius, tau, min_count, min_cos, stride, cut)
    geo = geometry.depth_geometry(pred, cameras, image, mask, space, **{k: opts[k] for k in geometry.DEFAULTS})
    B, H, W = geo["keep"].shape
    if B > 65535 or B * (-(-H // opts["stride"])) * (-(-W // opts["stride"])) >= MAX_NODES:
        raise ValueError(f"at most 65535 images and B * gh * gw < 2^30, got {(B, H, W)} at stride {opts['stride']}")
    if image is not None:
        image = np.asarray(image).reshape(B, 3, H, W)
    out = {k: geo[k] for k in ("xyz", "normal", "keep")}
    parts, v_off, f_off = [], [0], [0]
    for i in range(B):
        parts.append(mesh_from_planes(geo["xyz"][i], geo["normal"][i], geo["keep"][i], None if image is None else image[i], opts["stride"], opts["cut"]))
        v_off.append(v_off[-1] + len(parts[-1][0]))
        f_off.append(f_off[-1] + len(parts[-1][5]))
    for j, name in enumerate(MESH_ARRAYS):
        out[name] = np.concatenate([p[j] for p in parts])
    out["vertex_offsets"], out["face_offsets"] = np.array(v_off, np.int64), np.array(f_off, np.int64)
    return out


# ---- writers ----------------------------------------------------------------------------------------------------------------------------
def _mesh_arrays(vertices, normals, faces):
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    n = len(vertices)
    if vertices.shape != (n, 3) or faces.ndim != 2 or faces.shape[1:] != (3,) or faces.dtype.kind not in "iu":
        raise ValueError(f"vertices float [n, 3] and faces integers [m, 3], got {vertices.shape} and {faces.dtype} {faces.shape}")
    if normals is not None and np.shape(normals) != (n, 3):
        raise ValueError(f"normals float [n, 3] with n = {n}, got {np.shape(normals)}")
    if faces.size and (faces.min() < 0 or faces.max() >= n):
        raise ValueError(f"faces index the {n} vertices, got {int(faces.min())} .. {int(faces.max())}")
    return vertices.astype("<f4"), None if normals is None else np.asarray(normals).astype("<f4"), faces.astype("<u4")


def _png_bytes(image) -> bytes:
    import io
    from PIL import Image
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[0] != 3:
        raise ValueError(f"image: uint8 [3, H, W], got {image.dtype} {image.shape}")
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(image.transpose(1, 2, 0))).save(buf, format="PNG")
    return buf.getvalue()


def write_glb(path: str, vertices, normals, uv, faces, image=None, rgb=None) -> None:
    """One image's mesh as a binary glTF 2.0 file: one mesh with one primitive, POSITION (with min / max), NORMAL where given, TEXCOORD_0,
    uint32 indices.  With an `image` (uint8 [3, H, W]) the picture is embedded as a PNG and is the material's baseColorTexture; otherwise the
    primitive carries `rgb` (uint8 [n, 3]; white without it) as COLOR_0.  The material is double-sided, metallic 0, roughness 1.  glTF's axes
    are x right, y up, z to the viewer: positions and normals are written as (x, -y, -z), a half turn about x, so the winding stands and the
    front is counter-clockwise.  A mesh without faces gives a valid file whose scene has no mesh."""
    vertices, normals, faces = _mesh_arrays(vertices, normals, faces)
    n, m = len(vertices), len(faces)
    uv = np.asarray(uv).astype("<f4")
    if uv.shape != (n, 2):
        raise ValueError(f"uv float [n, 2] with n = {n}, got {uv.shape}")
    if rgb is not None and (np.shape(rgb) != (n, 3) or np.asarray(rgb).dtype != np.uint8):
        raise ValueError(f"rgb uint8 [n, 3] with n = {n}, got {np.asarray(rgb).dtype} {np.shape(rgb)}")
    png = _png_bytes(image) if image is not None else None
    flip = np.array([1.0, -1.0, -1.0], "<f4")
    gltf: Dict = dict(asset=dict(version="2.0", generator="genpercept_amd.mesh"), scene=0, scenes=[dict()])
    chunks, views, accessors = [], [], []

    def view(data: bytes, target: Optional[int] = None) -> int:
        offset = sum(len(c) for c in chunks)
        chunks.append(data + b"\0" * (-len(data) % 4))
        views.append(dict(buffer=0, byteOffset=offset, byteLength=len(data), **({} if target is None else dict(target=target))))
        return len(views) - 1

    def accessor(arr, kind: str, component: int, target: int, **extra) -> int:
        accessors.append(dict(bufferView=view(arr.tobytes(), target), componentType=component, count=len(arr) if arr.ndim > 1 else arr.size, type=kind, **extra))
        return len(accessors) - 1

    if m:
        pos = np.ascontiguousarray(vertices * flip)
        attributes = dict(POSITION=accessor(pos, "VEC3", 5126, 34962, min=[float(x) for x in pos.min(0)], max=[float(x) for x in pos.max(0)]))
        if normals is not None:
            attributes["NORMAL"] = accessor(np.ascontiguousarray(normals * flip), "VEC3", 5126, 34962)
        attributes["TEXCOORD_0"] = accessor(np.ascontiguousarray(uv), "VEC2", 5126, 34962)
        material: Dict = dict(doubleSided=True, pbrMetallicRoughness=dict(metallicFactor=0.0, roughnessFactor=1.0))
        if png is None:
            colour = np.full((n, 4), 255, np.uint8)
            if rgb is not None:
                colour[:, :3] = rgb
            attributes["COLOR_0"] = accessor(colour, "VEC4", 5121, 34962, normalized=True)
        indices = accessor(faces.reshape(-1), "SCALAR", 5125, 34963)
        if png is not None:
            gltf["images"] = [dict(bufferView=view(png), mimeType="image/png")]
            gltf["samplers"] = [dict(magFilter=9729, minFilter=9729, wrapS=33071, wrapT=33071)]
            gltf["textures"] = [dict(sampler=0, source=0)]
            material["pbrMetallicRoughness"]["baseColorTexture"] = dict(index=0)
        gltf.update(scenes=[dict(nodes=[0])], nodes=[dict(mesh=0)], materials=[material],
                    meshes=[dict(primitives=[dict(attributes=attributes, indices=indices, material=0, mode=4)])], accessors=accessors, bufferViews=views)
    body = b"".join(chunks)
    if body:
        gltf["buffers"] = [dict(byteLength=len(body))]
    text = json.dumps(gltf, separators=(",", ":")).encode("ascii")
    text += b" " * (-len(text) % 4)
    total = 12 + 8 + len(text) + (8 + len(body) if body else 0)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, total) + struct.pack("<I4s", len(text), b"JSON") + text)
        if body:
            f.write(struct.pack("<I4s", len(body), b"BIN\0") + body)


def write_mesh_ply(path: str, vertices, normals, rgb, faces) -> None:
    """One image's mesh as a binary little-endian PLY file: the vertex record of `geometry.write_ply` (x y z nx ny nz float, red green blue
    uchar, 27 bytes), then per face a uchar 3 and three int vertex indices."""
    vertices, normals, faces = _mesh_arrays(vertices, normals if normals is not None else np.zeros_like(np.asarray(vertices)), faces)
    n, m = len(vertices), len(faces)
    rgb = np.asarray(rgb)
    if rgb.shape != (n, 3) or rgb.dtype != np.uint8:
        raise ValueError(f"rgb uint8 [n, 3] with n = {n}, got {rgb.dtype} {rgb.shape}")
    rec = np.empty(n, geometry.PLY_DTYPE)
    for j, k in enumerate("xyz"):
        rec[k], rec["n" + k] = vertices[:, j], normals[:, j]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    face_rec = np.empty(m, np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    face_rec["n"], face_rec["v"] = 3, faces
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n"
    header += "".join(f"property float {k}\n" for k in ("x", "y", "z", "nx", "ny", "nz"))
    header += "".join(f"property uchar {k}\n" for k in ("red", "green", "blue"))
    header += f"element face {m}\nproperty list uchar int vertex_indices\nend_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + rec.tobytes() + face_rec.tobytes())
