"""numpy model of the thin-lens camera (acn_lens_rays, acn_render_lens): the expressions of include/actinon_hip.h in the header's
order, vectorised over ( position, sample ).  numpy's elementwise + - * / are IEEE binary64 and never contracted; sqrt goes through
the host build of csrc/acn_detmath.h (the `detmath_cpu` fixture of conftest.py), the LCG is integer arithmetic in uint64 and the
seeds come from the oracle's v3_random_seed (`oracle.random_seed`), so the device is compared with this model bit for bit."""
import numpy as np

JITTER = 1
DEFAULT_SAMPLES, MAX_SAMPLES, SEED, ROUNDS = 16, 4096, 2718281828, 32
LCG00_A, LCG00_C = np.uint64(6364136223846793005), np.uint64(1442695040888963407)    # ACN_LCG00_* of include/actinon_hip.h
RND0_SCALE, RND1_SCALE = 2.0 / float(0xFFFFFFFFFFFFFFFF), 1.0 / float(0xFFFFFFFFFFFFFFFF)
OP_SQRT = 7         # op code of tests/csrc/detmath_cpu.c


def sqrt(lib, x):
    shape = np.shape(x)
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.detmath_eval(OP_SQRT, x.ctypes.data, None, out.ctypes.data, x.size)
    return out.reshape(shape)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def of_length(lib, v, a):
    """v_of_length: unchanged when | |v|^2 - 1 | < 1e-8"""
    v = np.asarray(v, dtype=np.float64)
    r = dot(v, v)
    with np.errstate(all="ignore"):
        f = np.where(r > 0, a / sqrt(lib, r), 0.0)
    return np.where((np.abs(r - 1.0) < 1e-8)[..., None], v, v * f[..., None])


def cross(o, f):
    return np.stack([o[..., 1] * f[..., 2] - o[..., 2] * f[..., 1], o[..., 2] * f[..., 0] - o[..., 0] * f[..., 2],
                     o[..., 0] * f[..., 1] - o[..., 1] * f[..., 0]], axis=-1)


def m_mlv(m, v):
    """rows of m times v, each ( m.x * v.x + m.y * v.y ) + m.z * v.z"""
    v = np.asarray(v, dtype=np.float64)
    return np.stack([(m[i, 0] * v[..., 0] + m[i, 1] * v[..., 1]) + m[i, 2] * v[..., 2] for i in range(3)], axis=-1)


class Camera:
    """the camera basis of k_camera_setup and camera_ray (src/scene.c:963-990) of a scene's acn_params"""

    def __init__(self, lib, prm):
        self.lib = lib
        self.width, self.height = int(prm.image_width), int(prm.image_height)
        self.focal = float(prm.camera_focal_length)
        self.position = np.array(prm.camera_position[:], dtype=np.float64)
        self.unit_f = 1.0 / float(self.height >> 1)
        ry = of_length(lib, np.array(prm.camera_view_direction[:]), 1.0)
        rz = of_length(lib, np.array(prm.camera_top_direction[:]), 1.0)
        o_n = of_length(lib, ry, 1.0)                                         # v_von( ry, rz )
        rz = of_length(lib, rz - o_n * dot(o_n, rz), 1.0)
        rx = cross(ry, rz)
        self.rotation = np.stack([rx, ry, rz]).T.copy()                       # m_transposed
        self.R = m_mlv(self.rotation, np.array([1.0, 0.0, 0.0]))
        self.V = m_mlv(self.rotation, np.array([0.0, 1.0, 0.0]))
        self.T = m_mlv(self.rotation, np.array([0.0, 0.0, 1.0]))

    def rays(self, qx, qy):
        """camera_ray of positions ( qx, qy ) (arrays of one shape) -> origins, directions [..., 3]"""
        z = self.unit_f * (float(self.height >> 1) - qy)
        x = self.unit_f * (qx - float(self.width >> 1))
        d = of_length(self.lib, np.stack([x, np.full_like(x, self.focal), z], axis=-1), 1.0)
        return np.broadcast_to(self.position, d.shape).copy(), m_mlv(self.rotation, d)


def lcg(rv):
    with np.errstate(over="ignore"):
        return rv * LCG00_A + LCG00_C


def rnd0(rv):
    """f3_rnd0: one LCG step -> the new state, a number in [ -1, 1 ]"""
    rv = lcg(rv)
    return rv, rv.astype(np.float64) * RND0_SCALE - 1.0


def rnd1(rv):
    """f3_rnd1: one LCG step -> the new state, a number in [ 0, 1 ]"""
    rv = lcg(rv)
    return rv, rv.astype(np.float64) * RND1_SCALE


def seeds(oracle, pos, ks, seed):
    """v_random_seed( ( px, py, 2 k + 1 ), ACN_LENS_SEED + seed ) -> uint64 [n, len(ks)]"""
    s = (SEED + int(seed)) & 0xFFFFFFFFFFFFFFFF
    return np.array([[oracle.random_seed((p[0], p[1], float(2 * k + 1)), s) for k in ks] for p in pos], dtype=np.uint64).reshape(len(pos), len(ks))


def lens_rays(lib, oracle, prm, pos, samples=None, aperture=0.0, focus=0.0, jitter=False, seed=0, first_sample=0, n_samples=None,
              detail=None):
    """-> rays [n, n_samples, 6].  detail (a dict) receives what the rays were made of: the jittered positions q [n,s,2], the disc
    sample uv [n,s,2], the rounds drawn [n,s], the focus points F [n,s,3], the pinhole rays [n,s,6]"""
    samples = DEFAULT_SAMPLES if not samples else samples
    n_samples = samples - first_sample if n_samples is None else n_samples
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 2)
    ks = list(range(first_sample, first_sample + n_samples))
    cam = Camera(lib, prm)
    rv = seeds(oracle, pos, ks, seed)
    px = np.repeat(pos[:, 0:1], n_samples, axis=1)
    py = np.repeat(pos[:, 1:2], n_samples, axis=1)
    qx, qy = px, py
    if jitter:
        rv, a = rnd1(rv)
        jx = a - 0.5
        rv, a = rnd1(rv)
        jy = a - 0.5
        qx, qy = px + jx, py + jy
    o, d = cam.rays(qx, qy)
    info = {"q": np.stack([qx, qy], axis=-1), "pinhole": np.concatenate([o, d], axis=-1)}
    if aperture != 0.0:
        u, v = np.zeros_like(px), np.zeros_like(px)
        taken = np.zeros(px.shape, dtype=bool)
        rounds = np.zeros(px.shape, dtype=np.int64)
        for _ in range(ROUNDS):
            if taken.all():
                break
            r1, a = rnd0(rv)
            r2, b = rnd0(r1)
            rv = np.where(taken, rv, r2)                  # a lane that has its pair draws no more
            rounds = rounds + ~taken
            ok = ~taken & (a * a + b * b <= 1.0)
            u, v = np.where(ok, a, u), np.where(ok, b, v)
            taken = taken | ok
        t = focus / dot(d, cam.V)
        F = o + d * t[..., None]
        o = o + (cam.R * (aperture * u)[..., None] + cam.T * (aperture * v)[..., None])
        d = of_length(lib, F - o, 1.0)
        info.update(uv=np.stack([u, v], axis=-1), rounds=rounds, taken=taken, F=F)
    if detail is not None:
        detail.update(info)
    return np.concatenate([o, d], axis=-1)


def ordered_mean(L):
    """L [n, K, 3] -> ( ( ( 0.0 + L0 ) + L1 ) + ... ) / K"""
    s = np.zeros((L.shape[0], 3))
    for k in range(L.shape[1]):
        s = s + L[:, k]
    return s / float(L.shape[1])
