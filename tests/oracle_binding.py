"""ctypes binding of the CPU oracle (oracle/libacn_oracle*.so).  TEST INFRASTRUCTURE: only tests/, bench.py's
cpu_baseline leg and __graft_entry__.smoke() import this."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTER_NAMES = ["lum", "trans_ray", "shadow_ray", "obj_hit", "env_test", "plane_hit", "sphere_hit", "squaroid_hit",
                 "sdf_ray", "sdf_eval", "pair_hit", "side", "cap_sample", "oren_nayar", "fresnel", "node_visit", "flop", "transc",
                 # appended (oracle/acn_oracle.h): the two loops of scene_s_lum apart, and the part of flop / transc that scene_s_lum
                 # and the camera ray book themselves -- what is left, flop - flop_shade, is geometry
                 "oren_nayar_direct", "oren_nayar_path", "flop_shade", "transc_shade"]


class Oracle:
    def __init__(self, libm=False, path=None):
        name = "libacn_oracle_libm.so" if libm else "libacn_oracle.so"
        path = path or os.path.join(ROOT, "oracle", name)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `make oracle`")
        self.lib = C.CDLL(path)
        L = self.lib
        vp = C.c_void_p
        L.acn_oracle_render_positions.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, vp]
        L.acn_oracle_render_positions_shard.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, vp, C.c_uint32, C.c_uint32]
        L.acn_oracle_render_positions_work.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_int, vp, C.c_size_t, C.c_uint32, C.c_uint32]
        L.acn_oracle_estimate_envelope.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint32, C.c_double, vp]
        L.acn_oracle_sphere_ray_hit.argtypes = [vp, C.c_double, vp, vp, vp]
        L.acn_oracle_sphere_ray_hit.restype = C.c_double
        L.acn_oracle_plane_ray_hit.argtypes = [vp, vp, vp, vp]
        L.acn_oracle_plane_ray_hit.restype = C.c_double
        L.acn_oracle_fresnel_reflection.argtypes = [vp, vp, C.c_double, vp]
        L.acn_oracle_fresnel_reflection.restype = C.c_double
        L.acn_oracle_fresnel_refraction.argtypes = [vp, vp, C.c_double, vp]
        L.acn_oracle_fresnel_refraction.restype = None
        L.acn_oracle_obj_ray_hit.argtypes = [vp, C.c_int32, vp, vp, vp]
        L.acn_oracle_obj_ray_hit.restype = C.c_double
        L.acn_oracle_obj_side.argtypes = [vp, C.c_int32, vp]
        L.acn_oracle_trans_hit.argtypes = [vp, vp, vp, vp, vp, vp]
        L.acn_oracle_trans_hit.restype = C.c_double
        L.acn_oracle_random_seed.argtypes = [vp, C.c_uint64]
        L.acn_oracle_random_seed.restype = C.c_uint64
        L.acn_oracle_sphere_cap.argtypes = [vp, C.c_double, vp]
        L.acn_oracle_sphere_cap.restype = None
        L.acn_oracle_query_rays.argtypes = [vp, C.c_int, C.c_int32, vp, C.c_size_t, vp, vp, C.c_int]
        L.acn_oracle_shade_point.argtypes = [vp, vp, vp, C.c_size_t, vp, vp]
        L.acn_oracle_query_rays_counted.argtypes = [vp, C.c_int, C.c_int32, vp, C.c_size_t, vp, vp, C.c_int, vp]
        L.acn_oracle_shade_point_counters.argtypes = [vp, vp, vp]

    def math_mode(self):
        return self.lib.acn_oracle_math_mode()

    def render_positions(self, flat, pos_xy, linear=False, threads=None, counters=False, shard=None):
        """shard = (rank, world): this rank's share of a sample-sharded call (ACN_SHARD_SAMPLES); linear only."""
        pos = np.ascontiguousarray(pos_xy, dtype=np.float64).reshape(-1, 2)
        out = np.empty((pos.shape[0], 3), dtype=np.float64)
        cnt = (C.c_uint64 * len(COUNTER_NAMES))() if counters else None
        threads = threads or os.cpu_count() or 1
        rank, world = shard if shard else (0, 1)
        st = self.lib.acn_oracle_render_positions_work(C.addressof(flat.c), pos.ctypes.data, pos.shape[0], out.ctypes.data,
                                                       1 if linear else 0, threads, cnt, len(COUNTER_NAMES), rank, world)
        if st != 0:
            raise RuntimeError(f"oracle status {st}")
        if counters:
            return out, dict(zip(COUNTER_NAMES, [int(v) for v in cnt]))
        return out

    def estimate_envelope(self, flat, node, samples=1000, rseed=123, radius_factor=1.1):
        out = (C.c_double * 4)()
        st = self.lib.acn_oracle_estimate_envelope(C.addressof(flat.c), node, samples, rseed, radius_factor, out)
        if st != 0:
            raise RuntimeError(f"oracle status {st}")
        return list(out)

    @staticmethod
    def _a(v):
        return np.ascontiguousarray(v, dtype=np.float64)

    def sphere_ray_hit(self, pos, r, rp, rd):
        pos, rp, rd, nor = self._a(pos), self._a(rp), self._a(rd), np.zeros(3)
        a = self.lib.acn_oracle_sphere_ray_hit(pos.ctypes.data, r, rp.ctypes.data, rd.ctypes.data, nor.ctypes.data)
        return a, nor

    def plane_ray_hit(self, pos, nor, rp, rd):
        pos, nor, rp, rd = self._a(pos), self._a(nor), self._a(rp), self._a(rd)
        return self.lib.acn_oracle_plane_ray_hit(pos.ctypes.data, nor.ctypes.data, rp.ctypes.data, rd.ctypes.data)

    def fresnel_reflection(self, d, n, trix):
        d, n, out = self._a(d), self._a(n), np.zeros(3)
        r = self.lib.acn_oracle_fresnel_reflection(d.ctypes.data, n.ctypes.data, trix, out.ctypes.data)
        return r, out

    def fresnel_refraction(self, d, n, trix):
        d, n, out = self._a(d), self._a(n), np.zeros(3)
        self.lib.acn_oracle_fresnel_refraction(d.ctypes.data, n.ctypes.data, trix, out.ctypes.data)
        return out

    def obj_ray_hit(self, flat, node, rp, rd):
        rp, rd, nor = self._a(rp), self._a(rd), np.zeros(3)
        a = self.lib.acn_oracle_obj_ray_hit(C.addressof(flat.c), node, rp.ctypes.data, rd.ctypes.data, nor.ctypes.data)
        return a, nor

    def obj_side(self, flat, node, pos):
        pos = self._a(pos)
        return self.lib.acn_oracle_obj_side(C.addressof(flat.c), node, pos.ctypes.data)

    def trans_hit(self, flat, rp, rd):
        rp, rd, nor = self._a(rp), self._a(rd), np.zeros(3)
        ex, en = C.c_int32(-1), C.c_int32(-1)
        a = self.lib.acn_oracle_trans_hit(C.addressof(flat.c), rp.ctypes.data, rd.ctypes.data, nor.ctypes.data,
                                          C.byref(ex), C.byref(en))
        return a, nor, ex.value, en.value

    def random_seed(self, v, rv):
        v = self._a(v)
        return self.lib.acn_oracle_random_seed(v.ctypes.data, rv)

    def sphere_cap(self, rv, h):
        s = C.c_uint64(rv)
        out = np.zeros(3)
        self.lib.acn_oracle_sphere_cap(C.byref(s), h, out.ctypes.data)
        return s.value, out

    QUERY_OPS = {"obj_ray_hit": 0, "obj_side": 1, "compound_ray_hit": 2, "trans_hit": 3, "occluded": 4}

    def query_rays(self, flat, op, node, rays, limits=None, threads=16, counters=False):
        """acn_oracle_query_rays: [n, 8] results of the one-ray function `op` for rays [n, 6] (origin, direction).  counters: also
        the oracle's event counters of exactly these calls, as a dict (COUNTER_NAMES)."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        lim = None if limits is None else np.ascontiguousarray(limits, dtype=np.float64).reshape(-1)
        out = np.zeros((max(r.shape[0], 1), 8), dtype=np.float64)
        cnt = (C.c_uint64 * len(COUNTER_NAMES))() if counters else None
        st = self.lib.acn_oracle_query_rays_counted(C.addressof(flat.c), self.QUERY_OPS[op], int(node), r.ctypes.data, r.shape[0],
                                                    None if lim is None else lim.ctypes.data, out.ctypes.data, min(threads, 16), cnt)
        if st != 0:
            raise RuntimeError(f"oracle status {st}")
        if counters:
            return out[:r.shape[0]], dict(zip(COUNTER_NAMES, [int(v) for v in cnt]))
        return out[:r.shape[0]]

    def obj_ray_hits(self, flat, node, rays, threads=16):
        o = self.query_rays(flat, "obj_ray_hit", node, rays, threads=threads)
        return o[:, 0], o[:, 1:4]

    def obj_sides(self, flat, node, pos, threads=16):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        rays = np.concatenate([pos, np.zeros_like(pos)], axis=1)
        return self.query_rays(flat, "obj_side", node, rays, threads=threads)[:, 0].astype(np.int64)

    def compound_ray_hits(self, flat, node, rays, threads=16):
        o = self.query_rays(flat, "compound_ray_hit", node, rays, threads=threads)
        return o[:, 0], o[:, 1:4], o[:, 4].astype(np.int64)

    def trans_hits(self, flat, node, rays, threads=16):
        o = self.query_rays(flat, "trans_hit", node, rays, threads=threads)
        return o[:, 0], o[:, 1:4], o[:, 4].astype(np.int64), o[:, 5].astype(np.int64)

    # the rows of acn_oracle_shade_point (oracle/acn_oracle.h)
    TAP = {"emission": 0, "surface": 1, "fresnel": 2, "chromatic": 3, "refraction": 4, "diffuse": 5, "light": 6, "direct": 7, "paths": 8,
           "path": 9, "absorb": 10}
    TAP_STRIDE = 16

    def shade_point(self, flat, hit):
        """scene_s_lum for one hit without recursing: (rows [k, 16], lum [3]).  hit: [14] ray origin, direction, offs, exit normal,
        exit object, enter object, depth, intensity."""
        hit = np.ascontiguousarray(hit, dtype=np.float64).reshape(14)
        lum, n = np.zeros(3), C.c_size_t(0)
        room = 64
        while True:
            rows = np.zeros((room, self.TAP_STRIDE), dtype=np.float64)
            st = self.lib.acn_oracle_shade_point(C.addressof(flat.c), hit.ctypes.data, rows.ctypes.data, room, C.byref(n), lum.ctypes.data)
            if st != 0:
                raise RuntimeError(f"oracle status {st}")
            if n.value <= room:
                return rows[:n.value], lum
            room = n.value

    def shade_point_counters(self, flat, hit):
        """the oracle's event counters (COUNTER_NAMES) of the scene_s_lum call shade_point taps: its own events, and the geometry of
        its two sample loops (light hits, shadow rays, path transition hits); no specular child is traced"""
        hit = np.ascontiguousarray(hit, dtype=np.float64).reshape(14)
        cnt = (C.c_uint64 * len(COUNTER_NAMES))()
        st = self.lib.acn_oracle_shade_point_counters(C.addressof(flat.c), hit.ctypes.data, cnt)
        if st != 0:
            raise RuntimeError(f"oracle status {st}")
        return dict(zip(COUNTER_NAMES, [int(v) for v in cnt]))
