"""Moving an object of a flat scene: the frames of an animation for Handle.replace (acn_scene_replace) and motion_from_scenes.

rigid_copy restates acn_obj_rotate and acn_obj_move of actinon_amd/host/acn_scene.c on the nodes of a flat scene -- the same
expressions in the same order, in Python floats (IEEE binary64, never contracted), so the copy equals the flattened scene of the
object moved by the host library byte for byte."""
import ctypes as C

from . import abi
from .scene import Flat


def copy_flat(flat):
    """A Flat of its own arrays with the bytes of `flat`"""
    f = Flat()
    c = flat.c
    n, ne, nt = int(c.n_nodes), int(c.n_elems), int(c.n_textures)
    f._nodes = (abi.Node * max(1, n)).from_buffer_copy(flat.nodes_bytes().ljust(C.sizeof(abi.Node), b"\0"))
    f._elems = (C.c_int32 * max(1, ne))(*[c.elems[k] for k in range(ne)])
    tb = C.string_at(c.textures, C.sizeof(abi.Texture) * nt) if nt else b""
    f._tex = (abi.Texture * max(1, nt)).from_buffer_copy(tb.ljust(C.sizeof(abi.Texture), b"\0"))
    f.c.abi_version, f.c.n_nodes, f.c.n_elems, f.c.n_textures = c.abi_version, n, ne, nt
    f.c.light_root, f.c.matter_root = c.light_root, c.matter_root
    f.c.nodes = C.cast(f._nodes, C.POINTER(abi.Node))
    f.c.elems = C.cast(f._elems, C.POINTER(C.c_int32))
    f.c.textures = C.cast(f._tex, C.POINTER(abi.Texture))
    C.memmove(C.addressof(f.c.params), C.addressof(c.params), C.sizeof(abi.Params))
    if hasattr(flat, "driver"):
        f.driver = flat.driver
    return f


def m_mlv(m, v):
    """m_mlv of acn_scene.c: the rows of m times v, each sum from the left"""
    return [m[0][0] * v[0] + m[0][1] * v[1] + m[0][2] * v[2],
            m[1][0] * v[0] + m[1][1] * v[1] + m[1][2] * v[2],
            m[2][0] * v[0] + m[2][1] * v[1] + m[2][2] * v[2]]


def subtree(flat, node):
    """-> [( index, prp )]: the nodes acn_obj_move / acn_obj_rotate reach from `node`, in their order; prp False for a compound, of
    which only the envelope moves.  Compound elements, both operands of a pair, the operand of a neg; a scale node itself only"""
    out, todo = [], [int(node)]
    while todo:
        i = todo.pop()
        nd = flat.c.nodes[i]
        out.append((i, nd.type != abi.ACN_COMPOUND))
        if nd.type == abi.ACN_COMPOUND:
            todo.extend(reversed(flat.elems_of(i)))
        elif nd.type in (abi.ACN_PAIR_INSIDE, abi.ACN_PAIR_OUTSIDE):
            todo.extend((nd.child1, nd.child0))
        elif nd.type == abi.ACN_NEG:
            todo.append(nd.child0)
    return out


def rigid_copy(flat, node, rotation3x3=None, pivot=None, shift=None):
    """A copy of `flat` in which the subtree of node index `node` is turned by rotation3x3 (rows x, y, z) about `pivot` (default: the
    origin) and then shifted by `shift`: per node acn_obj_move( -pivot ), acn_obj_rotate( rotation ), acn_obj_move( pivot ),
    acn_obj_move( shift ) on pos, rax and, where the node has one, the envelope's position.  None leaves a step out."""
    if not 0 <= int(node) < flat.c.n_nodes:
        raise ValueError(f"node {node} is not one of the scene's {flat.c.n_nodes}")
    out = copy_flat(flat)
    mat = None if rotation3x3 is None else [[float(v) for v in row] for row in rotation3x3]
    steps = []
    if mat is not None:
        if pivot is not None:
            steps.append(("move", [-float(v) for v in pivot]))
        steps.append(("rotate", mat))
        if pivot is not None:
            steps.append(("move", [float(v) for v in pivot]))
    if shift is not None:
        steps.append(("move", [float(v) for v in shift]))
    for i, prp in subtree(out, node):
        nd = out.c.nodes[i]
        has_env = bool(nd.flags & abi.ACN_NODE_HAS_ENVELOPE)
        for kind, arg in steps:
            if kind == "move":
                if prp:
                    nd.pos[:] = [nd.pos[k] + arg[k] for k in range(3)]
                if has_env:
                    nd.env_pos[:] = [nd.env_pos[k] + arg[k] for k in range(3)]
            else:
                if prp:
                    rows = [m_mlv(arg, list(nd.rax[3 * r:3 * r + 3])) for r in range(3)]     # m_mlm: every row of rax turned
                    nd.rax[:] = rows[0] + rows[1] + rows[2]
                    nd.pos[:] = m_mlv(arg, list(nd.pos))
                if has_env:
                    nd.env_pos[:] = m_mlv(arg, list(nd.env_pos))
    return out


def rotation_about(axis, degrees):
    """The rotation by `degrees` about `axis` (any length but 0) as rows x, y, z: Rodrigues' formula"""
    import math
    x, y, z = (float(v) for v in axis)
    r = math.sqrt(x * x + y * y + z * z)
    if not r > 0:
        raise ValueError("the axis of a rotation has a length")
    x, y, z = x / r, y / r, z / r
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    t = 1.0 - c
    return [[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
            [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
            [t * x * z - s * y, t * y * z + s * x, t * z * z + c]]
