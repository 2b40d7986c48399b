"""Host-side engine over one C-ABI handle: marshals numpy / torch buffers to the library.

PyTorch is used only as a tensor container (device memory, ``data_ptr()``); every computation
is a HIP kernel behind include/lwpose.h.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, check, lib

_ROLE_NBT = 6


def _torch():
    import torch
    return torch


class Engine(object):
    def __init__(self, device_id=0, nref=1, num_channels=128, num_heatmaps=19, num_pafs=38, dtype=_lib.F32):
        self.h = _lib.Handle(device_id, nref, num_channels, num_heatmaps, num_pafs, dtype)
        self.nref, self.C, self.NH, self.NP = nref, num_channels, num_heatmaps, num_pafs
        self.device_id = device_id
        self._keep = None
        self.stage_steps = 0                  # adam_step calls so far: the drop-in net reads its stage parameters back when this moves
        self.train_scope = "stages"           # set_train_scope: "stages" | "cpm" | "all"
        self._scope_steps = 0                 # stage_steps when the current scope was set
        self._left_params = {}                # parameters an earlier, wider scope trained and the current one does not cover
        self._coco_n = 0                      # images of the open detection store (coco_open); 0: none, the library reports it
        self._val_store = None

    # ------------------------------------------------------------------ stream ordering
    def _order(self, device=None, hand_over=True):
        """Order the library's stream against torch's CURRENT stream on this GPU with events (lwp_set_stream): no host block.
        The reference's net(x) runs on the current stream (demo.py:64-68); this gives device tensors the same semantics —
        inputs written by queued torch work are waited for, and torch work queued after the call sees the device results.
        ``hand_over=False``: results left on the device stay on the library's stream (for its own next call)."""
        torch = _torch()
        st = torch.cuda.current_stream(torch.device("cuda", self.device_id) if device is None else device)
        check(lib().lwp_set_stream(self.h.ptr, C.c_void_p(st.cuda_stream), 1 if hand_over else 2), self.h.ptr)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict):
        """state_dict: key -> torch tensor / numpy array (float32; num_batches_tracked int64)."""
        names, arrs = [], []
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            if a.dtype != np.int64:
                a = np.ascontiguousarray(a, dtype=np.float32)
            names.append(k.encode())
            arrs.append(np.ascontiguousarray(a))
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        shapes = np.ones((n, 4), dtype=np.int64)
        ndims = np.zeros(n, dtype=np.int32)
        for i, a in enumerate(arrs):
            ndims[i] = a.ndim
            shapes[i, :a.ndim] = a.shape
        check(lib().lwp_load_weights(self.h.ptr, c_names, c_ptrs, shapes.ctypes.data_as(C.POINTER(C.c_int64)),
                                     ndims.ctypes.data_as(C.POINTER(C.c_int)), n), self.h.ptr)
        self._left_params = {}                # every parameter has just been replaced
        self._scope_steps = self.stage_steps

    def weights_blob_bytes(self):
        n = C.c_size_t()
        check(lib().lwp_weights_blob_bytes(self.h.ptr, C.byref(n)), self.h.ptr)
        return n.value

    def export_weights(self, device_tensor):
        check(lib().lwp_weights_blob_export(self.h.ptr, device_tensor.data_ptr(), device_tensor.numel() * device_tensor.element_size()), self.h.ptr)

    def import_weights(self, device_tensor):
        check(lib().lwp_weights_blob_import(self.h.ptr, device_tensor.data_ptr(), device_tensor.numel() * device_tensor.element_size()), self.h.ptr)

    # ------------------------------------------------------------------ skeleton (modules/keypoints.py:5-8, group_keypoints' options)
    def set_skeleton(self, limb_kpts, limb_pafs, num_kpt_types=None, pose_entry_size=None, min_paf_score=0.05):
        """Grouping tables for a network trained on another key-point set: limb_kpts / limb_pafs are the L (a, b) key-point
        type pairs and their PAF channel pairs, in grouping order.  num_kpt_types defaults to num_heatmaps - 1,
        pose_entry_size to max(20, K + 2).  ``limb_kpts=None`` restores the COCO default.  Bad tables raise ValueError."""
        if limb_kpts is None:
            check(lib().lwp_set_skeleton(self.h.ptr, 0, 0, None, None, 0, 0.0), self.h.ptr)
            self._skel = None
            return
        kp = np.ascontiguousarray(np.asarray(limb_kpts, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
        pf = np.ascontiguousarray(np.asarray(limb_pafs, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
        if len(kp) == 0:                       # (an empty table is an error, not the default: that is limb_kpts=None)
            raise ValueError("a skeleton needs 1..320 limbs, got none")
        if len(kp) != len(pf):
            raise ValueError("limb_kpts and limb_pafs must have the same number of limbs (%d != %d)" % (len(kp), len(pf)))
        K = int(self.NH - 1 if num_kpt_types is None else num_kpt_types)
        E = int(max(20, K + 2) if pose_entry_size is None else pose_entry_size)
        check(lib().lwp_set_skeleton(self.h.ptr, K, len(kp), kp.ctypes.data_as(C.POINTER(C.c_int)), pf.ctypes.data_as(C.POINTER(C.c_int)),
                                     E, float(min_paf_score)), self.h.ptr)
        self._skel = None

    @property
    def skeleton(self):
        """dict(num_kpt_types, limb_kpts (L,2), limb_pafs (L,2), pose_entry_size, min_paf_score) of the handle."""
        if getattr(self, "_skel", None) is None:
            K, L, E, mp = C.c_int(), C.c_int(), C.c_int(), C.c_double()
            check(lib().lwp_get_skeleton(self.h.ptr, C.byref(K), C.byref(L), None, None, 0, C.byref(E), C.byref(mp)), self.h.ptr)
            kp = np.zeros((L.value, 2), np.int32)
            pf = np.zeros((L.value, 2), np.int32)
            check(lib().lwp_get_skeleton(self.h.ptr, None, None, kp.ctypes.data_as(C.POINTER(C.c_int)), pf.ctypes.data_as(C.POINTER(C.c_int)),
                                         L.value, None, None), self.h.ptr)
            self._skel = dict(num_kpt_types=K.value, limb_kpts=kp, limb_pafs=pf, pose_entry_size=E.value, min_paf_score=mp.value)
        return self._skel

    @property
    def post_generic(self):
        """True when the generic grouping kernels run (custom skeleton, or LWP_POST_GENERIC=1 at creation) — debug."""
        rc = lib().lwp_debug_post_generic(self.h.ptr)
        if rc < 0:
            check(rc, self.h.ptr)
        return rc == 1

    def set_capacity(self, max_peaks=2048, max_kpts=128, max_conn=4096, max_entries=256):
        check(lib().lwp_set_capacity(self.h.ptr, max_peaks, max_kpts, max_conn, max_entries), self.h.ptr)
        self._caps = (max_peaks, max_kpts, max_conn, max_entries)

    @property
    def caps(self):
        return getattr(self, "_caps", (2048, 128, 4096, 256))

    # ------------------------------------------------------------------ network
    def forward(self, x):
        """x: (N,3,H,W) float32 torch tensor (cpu or cuda) or numpy array -> list of 2(1+nref) outputs of the
        same kind (NCHW), like PoseEstimationWithMobileNet.forward (with_mobilenet.py:114-123)."""
        torch = _torch()
        is_np = isinstance(x, np.ndarray)
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if is_np else x
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError("expected input of shape (N, 3, H, W), got %s" % (tuple(t.shape),))
        t = t.detach().to(torch.float32).contiguous()
        N, _, H, W = t.shape
        on_dev = t.is_cuda
        if on_dev and t.device.index != self.device_id:
            raise ValueError("input is on cuda:%d but the engine lives on cuda:%d" % (t.device.index, self.device_id))
        fh, fw = H, W
        for _ in range(3):                       # three stride-2 stages: out = (in - 1) // 2 + 1
            fh, fw = (fh - 1) // 2 + 1, (fw - 1) // 2 + 1
        shapes = [(N, self.NP if i % 2 else self.NH, fh, fw) for i in range(2 * (1 + self.nref))]
        outs = [torch.empty(s, dtype=torch.float32, device=t.device) for s in shapes]
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        if on_dev:
            self._order(t.device)                 # events both ways: the outputs are valid for work queued on torch's current stream
            # (a frame from preprocess_u8(hand_over=False) is in order on the engine's stream; the outputs still need the hand-over)
        mem = MEM_DEVICE if on_dev else MEM_HOST
        check(lib().lwp_forward(self.h.ptr, t.data_ptr(), mem, N, H, W, ptrs, mem), self.h.ptr)
        return [o.numpy() for o in outs] if is_np else outs

    def synchronize(self):
        check(lib().lwp_synchronize(self.h.ptr), self.h.ptr)

    # ------------------------------------------------------------------ post-processing pieces
    def upsample(self, maps_nchw, ratio=4):
        """(N,C,h,w) float32 numpy -> (N, h*r, w*r, C) float32 numpy (cv2.resize INTER_CUBIC, demo.py:72,76)."""
        if getattr(maps_nchw, "is_cuda", False):
            a = maps_nchw.detach().contiguous()
            self._order(a.device)
            ptr, mem = a.data_ptr(), MEM_DEVICE
        else:
            a = np.ascontiguousarray(maps_nchw.numpy() if hasattr(maps_nchw, "numpy") else maps_nchw, dtype=np.float32)
            ptr, mem = a.ctypes.data, MEM_HOST
        N, Cc, h, w = a.shape
        out = np.empty((N, h * ratio, w * ratio, Cc), dtype=np.float32)
        check(lib().lwp_upsample(self.h.ptr, ptr, mem, N, Cc, h, w, ratio, out.ctypes.data, MEM_HOST), self.h.ptr)
        return out

    @staticmethod
    def preprocess_dims(height, width, net_input_height_size, stride):
        """(scaled_h, scaled_w, out_h, out_w, pad [top,left,bottom,right], scale) of demo.py:55-62 for a height x width frame."""
        v = [C.c_int() for _ in range(4)]
        pad = (C.c_int * 4)()
        sc = C.c_double()
        check(lib().lwp_preprocess_dims(height, width, net_input_height_size, stride, *[C.byref(a) for a in v], pad, C.byref(sc)))
        return v[0].value, v[1].value, v[2].value, v[3].value, [int(a) for a in pad], sc.value

    def preprocess_u8(self, img, net_input_height_size, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1 / 256,
                      hand_over=True):
        """uint8 HxWx3 frame (numpy or cuda tensor) -> (x: 1x3xH'xW' float32 cuda tensor, scale, pad): the cubic resize,
        normalize and pad_width of demo.py:55-64 in one kernel.  ``hand_over=False`` (infer_fast's internal use): x is only meant
        for this engine's next call — it stays on the engine's stream and that call skips the stream ordering (no events)."""
        torch = _torch()
        if getattr(img, "is_cuda", False):
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise TypeError("frame must be HxWx3 uint8")
            a = img.contiguous()
            ptr, mem = a.data_ptr(), MEM_DEVICE
        else:
            a = np.ascontiguousarray(img)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise TypeError("frame must be HxWx3 uint8")
            ptr, mem = a.ctypes.data, MEM_HOST
        H, W = int(a.shape[0]), int(a.shape[1])
        _, _, oh, ow, pad, scale = self.preprocess_dims(H, W, net_input_height_size, stride)
        x = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=torch.device("cuda", self.device_id))
        pv = (C.c_double * 3)(*[float(v) for v in pad_value])
        mv = (C.c_double * 3)(*[float(v) for v in img_mean])
        self._order(hand_over=hand_over)          # x is handed to torch's current stream by event; a host frame may be reused on return
        check(lib().lwp_preprocess_u8(self.h.ptr, ptr, mem, H, W, net_input_height_size, stride, pv, mv, float(img_scale), x.data_ptr()), self.h.ptr)
        if not hand_over:
            x._lwp_stream_owner = self            # produced on this engine's stream, not visible to torch's stream
        return x, scale, pad

    def _u8_frames(self, frames):
        """(pointer, mem flag, N, H, W, the array kept alive) of a uint8 frame batch (N,H,W,3) or one frame (H,W,3), numpy or a
        cuda tensor on this engine's GPU."""
        torch = _torch()
        on_dev = getattr(frames, "is_cuda", False)
        a = frames.contiguous() if on_dev else np.ascontiguousarray(frames)
        if a.dtype != (torch.uint8 if on_dev else np.uint8) or len(a.shape) not in (3, 4) or a.shape[-1] != 3:
            raise TypeError("frames must be (N,)HxWx3 uint8")
        shp = tuple(a.shape) if len(a.shape) == 4 else (1,) + tuple(a.shape)
        if on_dev:
            if a.device.index != self.device_id:
                raise ValueError("frames are on cuda:%d but the engine lives on cuda:%d" % (a.device.index, self.device_id))
            return a.data_ptr(), MEM_DEVICE, int(shp[0]), int(shp[1]), int(shp[2]), a
        return a.ctypes.data, MEM_HOST, int(shp[0]), int(shp[1]), int(shp[2]), a

    def preprocess_u8_batch(self, frames, net_input_height_size, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1 / 256,
                            hand_over=True):
        """N same-sized uint8 frames (N,H,W,3) or one (H,W,3), numpy or cuda tensor -> (x: N x 3 x H' x W' float32 cuda tensor,
        scale, pad): ``preprocess_u8`` for a batch in ONE launch (demo.py:55-64 per frame, same bits)."""
        torch = _torch()
        ptr, mem, N, H, W, a = self._u8_frames(frames)
        _, _, oh, ow, pad, scale = self.preprocess_dims(H, W, net_input_height_size, stride)
        x = torch.empty((N, 3, oh, ow), dtype=torch.float32, device=torch.device("cuda", self.device_id))
        pv = (C.c_double * 3)(*[float(v) for v in pad_value])
        mv = (C.c_double * 3)(*[float(v) for v in img_mean])
        self._order(hand_over=hand_over)
        check(lib().lwp_preprocess_u8_batch(self.h.ptr, ptr, mem, N, H, W, net_input_height_size, stride, pv, mv, float(img_scale),
                                            x.data_ptr()), self.h.ptr)
        if not hand_over:
            x._lwp_stream_owner = self
        return x, scale, pad

    @staticmethod
    def scale_dims(height, width, ratio, base_height, stride):
        """(scaled_h, scaled_w, out_h, out_w, pad [top,left,bottom,right]) of val.py:89-91 for a height x width frame."""
        v = [C.c_int() for _ in range(4)]
        pad = (C.c_int * 4)()
        check(lib().lwp_scale_dims(height, width, float(ratio), base_height, stride, *[C.byref(a) for a in v], pad))
        return v[0].value, v[1].value, v[2].value, v[3].value, [int(a) for a in pad]

    def preprocess_scaled_u8(self, imgs, ratio, base_height, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1 / 256):
        """N same-sized frames (N,H,W,3) or one (H,W,3), numpy or cuda tensor, uint8 or float32 -> (x: N x 3 x H' x W' float32
        cuda tensor, pad): normalize + cubic resize by ``ratio`` + pad_width of val.py:84-93 in one kernel."""
        torch = _torch()
        on_dev = getattr(imgs, "is_cuda", False)
        a = imgs.contiguous() if on_dev else np.ascontiguousarray(imgs)
        is_u8 = a.dtype == (torch.uint8 if on_dev else np.uint8)
        is_f32 = a.dtype == (torch.float32 if on_dev else np.float32)
        if not (is_u8 or is_f32) or len(a.shape) not in (3, 4) or a.shape[-1] != 3:
            raise TypeError("frames must be (N,)HxWx3 uint8 or float32")
        shp = tuple(a.shape) if len(a.shape) == 4 else (1,) + tuple(a.shape)
        N, H, W = int(shp[0]), int(shp[1]), int(shp[2])
        _, _, oh, ow, pad = self.scale_dims(H, W, ratio, base_height, stride)
        if on_dev:
            if a.device.index != self.device_id:
                raise ValueError("frames are on cuda:%d but the engine lives on cuda:%d" % (a.device.index, self.device_id))
            ptr, mem = a.data_ptr(), MEM_DEVICE
        else:
            ptr, mem = a.ctypes.data, MEM_HOST
        self._order()
        x = torch.empty((N, 3, oh, ow), dtype=torch.float32, device=torch.device("cuda", self.device_id))
        pv = (C.c_double * 3)(*[float(v) for v in pad_value])
        mv = (C.c_double * 3)(*[float(v) for v in img_mean])
        fn = lib().lwp_preprocess_scaled_u8 if is_u8 else lib().lwp_preprocess_scaled_f32
        check(fn(self.h.ptr, ptr, mem, N, H, W, float(ratio), base_height, stride, pv, mv, float(img_scale), x.data_ptr()), self.h.ptr)
        return x, pad

    def multiscale_accumulate(self, accum, maps, up_ratio, pad, n_scales, init=False):
        """accum (H,W,C) or (N,H,W,C) float32 [numpy or cuda tensor, updated in place] += resize(crop(upsample(maps))) / n_scales
        (val.py:96-101).  maps: (C,h,w) or (N,C,h,w) float32 numpy / cuda tensor; the N frames share pad and size.
        init=True: accum is treated as zero (first scale), so it may be uninitialised memory."""
        def ptr_mem(a):
            if getattr(a, "is_cuda", False):
                return a.data_ptr(), MEM_DEVICE
            return a.ctypes.data, MEM_HOST
        if getattr(maps, "is_cuda", False):
            maps = maps.detach().contiguous()
        else:
            maps = np.ascontiguousarray(maps, dtype=np.float32)
        shp = tuple(maps.shape)
        ashp = tuple(accum.shape)
        N = shp[0] if len(shp) == 4 else 1
        if len(ashp) not in (3, 4) or (len(ashp) == 4 and ashp[0] != N) or (len(ashp) == 3 and N != 1):
            raise ValueError("accum / maps batch mismatch")
        H, W, Cc = ashp[-3:]
        if Cc != shp[-3]:
            raise ValueError("channel mismatch")
        if getattr(accum, "is_cuda", False):
            if not accum.is_contiguous() or accum.dtype != _torch().float32:
                raise TypeError("accum must be a contiguous float32 tensor")
        elif accum.dtype != np.float32 or not accum.flags.c_contiguous:
            raise TypeError("accum must be a C-contiguous float32 array")
        mp, mm = ptr_mem(maps)
        ap, am = ptr_mem(accum)
        if mm == MEM_DEVICE or am == MEM_DEVICE:
            self._order()
        padv = (C.c_int * 4)(*[int(v) for v in pad])
        check(lib().lwp_multiscale_accumulate(self.h.ptr, mp, mm, N, shp[-3], shp[-2], shp[-1], up_ratio, padv, H, W, n_scales, ap, am, 1 if init else 0), self.h.ptr)
        return accum

    def extract_keypoints(self, heatmap):
        """In-place threshold of ``heatmap`` (2-D float32 view) and key-point list [(x, y, score)]."""
        if not isinstance(heatmap, np.ndarray) or heatmap.ndim != 2 or heatmap.dtype != np.float32:
            raise TypeError("heatmap must be a 2-D float32 numpy array (view)")
        if not heatmap.flags.writeable:
            raise ValueError("heatmap must be writeable (it is thresholded in place)")
        H, W = heatmap.shape
        if heatmap.strides[0] % 4 or heatmap.strides[1] % 4:
            raise ValueError("unsupported strides")
        cap = self.caps[1]
        xs = np.empty(cap, np.int64); ys = np.empty(cap, np.int64); sc = np.empty(cap, np.float32)
        n = C.c_int()
        check(lib().lwp_extract_keypoints(self.h.ptr, heatmap.ctypes.data, H, W, heatmap.strides[0] // 4, heatmap.strides[1] // 4,
                                          xs.ctypes.data_as(C.POINTER(C.c_int64)), ys.ctypes.data_as(C.POINTER(C.c_int64)),
                                          sc.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)), self.h.ptr)
        return xs[:n.value], ys[:n.value], sc[:n.value]

    def group_keypoints(self, kpts, type_counts, pafs, demo):
        """kpts (n,4) float64, type_counts (K,), pafs (H,W,num_pafs) float32 -> (P,E) float64 (K / E: the skeleton's, 18 / 20 by
        default)."""
        pafs = np.ascontiguousarray(pafs, dtype=np.float32)
        H, W, NPc = pafs.shape
        if NPc != self.NP:
            raise ValueError("pafs must have %d channels" % self.NP)
        kp = np.ascontiguousarray(kpts, dtype=np.float64).reshape(-1, 4)
        tc = np.ascontiguousarray(type_counts, dtype=np.int32)
        sk = self.skeleton
        if tc.shape != (sk["num_kpt_types"],):
            raise ValueError("type_counts must have %d entries (the skeleton's key-point types)" % sk["num_kpt_types"])
        cap = self.caps[3]
        ent = np.empty((cap, sk["pose_entry_size"]), np.float64)
        n = C.c_int()
        check(lib().lwp_group_keypoints(self.h.ptr, kp.ctypes.data, tc.ctypes.data_as(C.POINTER(C.c_int)), pafs.ctypes.data,
                                        MEM_HOST, H, W, 1 if demo else 0, ent.ctypes.data, cap, C.byref(n)), self.h.ptr)
        return ent[:n.value].copy()

    # ------------------------------------------------------------------ fused pipeline
    def _result_buffers(self, N):
        sk = self.skeleton
        K, E = sk["num_kpt_types"], sk["pose_entry_size"]
        kcap = K * self.caps[1]
        ecap = self.caps[3]
        return (np.zeros((N, K), np.int32), np.zeros((N, kcap, 4), np.float64), np.zeros((N, ecap, E), np.float64),
                np.zeros(N, np.int32), kcap, ecap)

    @staticmethod
    def _unpack(N, counts, kpts, ent, ne):
        out = []
        for f in range(N):
            K = int(counts[f].sum())
            out.append((ent[f, :ne[f]].copy(), kpts[f, :K].copy(), counts[f].copy()))
        return out

    def infer_poses(self, x, upsample_ratio=4, demo=True):
        """x: (N,3,H,W) float32 (numpy / cpu tensor / cuda tensor), already normalised and padded.
        Returns per frame (pose_entries (P,E) f64, all_keypoints (n,4) f64, type_counts (K,)); K / E of the skeleton (18 / 20 by
        default)."""
        torch = _torch()
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray) else x
        t = t.detach().to(torch.float32).contiguous()
        N, _, H, W = t.shape
        counts, kpts, ent, ne, kcap, ecap = self._result_buffers(N)
        if t.is_cuda and getattr(x, "_lwp_stream_owner", None) is not self:
            self._order(t.device)
        check(lib().lwp_infer_poses(self.h.ptr, t.data_ptr(), MEM_DEVICE if t.is_cuda else MEM_HOST, N, H, W, upsample_ratio,
                                    1 if demo else 0, counts.ctypes.data_as(C.POINTER(C.c_int)), kpts.ctypes.data, kcap,
                                    ent.ctypes.data, ecap, ne.ctypes.data_as(C.POINTER(C.c_int))), self.h.ptr)
        self._last_N = N
        return self._unpack(N, counts, kpts, ent, ne)

    def poses_from_maps(self, heat, paf, upsample_ratio=4, demo=True, layout="NCHW"):
        """Post-processing only.  layout "NCHW": the low-res stage outputs (N,19,h,w) / (N,38,h,w); layout "NHWC": full-res
        averaged maps (N,H,W,19) / (N,H,W,38) of the multi-scale path with upsample_ratio=1.  float32 numpy or cuda tensors."""
        lay = {"NCHW": 0, "NHWC": 1}[layout]
        if getattr(heat, "is_cuda", False):
            heat, paf = heat.detach().contiguous(), paf.detach().contiguous()
            self._order(heat.device)
            hp, pp, mem = heat.data_ptr(), paf.data_ptr(), MEM_DEVICE
        else:
            heat = np.ascontiguousarray(heat, dtype=np.float32)
            paf = np.ascontiguousarray(paf, dtype=np.float32)
            hp, pp, mem = heat.ctypes.data, paf.ctypes.data, MEM_HOST
        if lay == 0:
            N, _, hs, ws = heat.shape
        else:
            N, hs, ws, _ = heat.shape
        counts, kpts, ent, ne, kcap, ecap = self._result_buffers(N)
        check(lib().lwp_poses_from_maps(self.h.ptr, hp, pp, mem, lay, N, hs, ws, upsample_ratio,
                                        1 if demo else 0, counts.ctypes.data_as(C.POINTER(C.c_int)), kpts.ctypes.data, kcap,
                                        ent.ctypes.data, ecap, ne.ctypes.data_as(C.POINTER(C.c_int))), self.h.ptr)
        self._last_N = N
        return self._unpack(N, counts, kpts, ent, ne)

    def layers(self):
        out = []
        name = C.create_string_buffer(128)
        v = [C.c_int() for _ in range(6)]
        macs = C.c_int64()
        for i in range(lib().lwp_layer_count(self.h.ptr)):
            check(lib().lwp_layer_info(self.h.ptr, i, name, 128, *[C.byref(x) for x in v], C.byref(macs)), self.h.ptr)
            out.append(dict(index=i, name=name.value.decode(), kind=v[0].value, cin=v[1].value, cout=v[2].value,
                            ksize=v[3].value, stride=v[4].value, dilation=v[5].value, macs_per_pixel=macs.value))
        return out

    def debug_layer_output(self, x, layer_index):
        """Output of layer ``layer_index`` (NCHW float32 numpy) for input x (N,3,H,W) numpy."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        N, _, H, W = x.shape
        info = self.layers()[layer_index]
        buf = np.empty(N * info["cout"] * ((H + 1) // 2) * ((W + 1) // 2), np.float32)
        dims = (C.c_int * 4)()
        check(lib().lwp_debug_layer_output(self.h.ptr, x.ctypes.data, N, H, W, layer_index, buf.ctypes.data, buf.size, dims), self.h.ptr)
        n = dims[0] * dims[1] * dims[2] * dims[3]
        return buf[:n].reshape(dims[0], dims[1], dims[2], dims[3]).copy()

    def frames_per_pass(self, N, H, W):
        """Frames one launch sequence of an (N,3,H,W) call takes (N unless the batch is split inside the call)."""
        n = lib().lwp_debug_frames_per_pass(self.h.ptr, N, H, W)
        if n < 0:
            raise ValueError("bad shape")
        return n

    def post_counts(self, frame=0):
        """(peaks per type before the NMS [K], key-points per type [K], scored connection candidates per limb [L], picked
        connections per limb [L]) of one frame of the last infer_poses / poses_from_maps call (debug; 18 / 19 by default)."""
        sk = self.skeleton
        K, L = sk["num_kpt_types"], len(sk["limb_kpts"])
        arrs = [(C.c_int * n)() for n in (K, K, L, L)]
        check(lib().lwp_debug_post_counts_ex(self.h.ptr, frame, *arrs, K, L), self.h.ptr)
        return tuple(np.array(list(a), dtype=np.int64) for a in arrs)

    def layer_variant(self, layer_index):
        """Kernel variant the last debug_layer_output / profile_launches pass picked for a layer ("" before any)."""
        name = C.create_string_buffer(96)
        check(lib().lwp_debug_layer_variant(self.h.ptr, layer_index, name, 96), self.h.ptr)
        return name.value.decode()

    def _as_device_input(self, x):
        """Checks shared by every entry point that hands ``data_ptr()`` of a resident frame batch to the library: float32,
        contiguous, (N,3,H,W), on this engine's GPU; work still queued on torch's current stream is ordered before the
        library's (own, non-blocking) stream by an event — the host does not wait."""
        torch = _torch()
        if not getattr(x, "is_cuda", False):
            raise TypeError("expected a cuda tensor")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise TypeError("expected a float32 (N, 3, H, W) tensor, got %s %s" % (x.dtype, tuple(x.shape)))
        if not x.is_contiguous():
            raise ValueError("input tensor must be contiguous")
        if x.device.index != self.device_id:
            raise ValueError("input is on cuda:%d but the engine lives on cuda:%d" % (x.device.index, self.device_id))
        if getattr(x, "_lwp_stream_owner", None) is not self:     # (a tensor this engine produced on its own stream is in order already)
            self._order(x.device)
        return x

    def infer_poses_async(self, x_cuda, upsample_ratio=4, demo=True):
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        self._keep = x_cuda
        check(lib().lwp_infer_poses_async(self.h.ptr, x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0), self.h.ptr)
        self._last_N = N

    def fetch_poses(self):
        N = self._last_N
        counts, kpts, ent, ne, kcap, ecap = self._result_buffers(N)
        check(lib().lwp_fetch_poses(self.h.ptr, counts.ctypes.data_as(C.POINTER(C.c_int)), kpts.ctypes.data, kcap, ent.ctypes.data,
                                    ecap, ne.ctypes.data_as(C.POINTER(C.c_int))), self.h.ptr)
        return self._unpack(N, counts, kpts, ent, ne)

    # ------------------------------------------------------------------ pipelined streaming (two slots)
    def pipeline_submit(self, x_cuda, slot, upsample_ratio=4, demo=True):
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        self._keep_slot = getattr(self, "_keep_slot", {})
        self._keep_slot[slot] = (x_cuda, N)
        check(lib().lwp_pipeline_submit(self.h.ptr, x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, slot), self.h.ptr)

    def pipeline_submit_u8(self, frames, slot, net_input_height_size, stride=8, pad_value=(0, 0, 0), img_mean=(128, 128, 128),
                           img_scale=1 / 256, upsample_ratio=4, demo=True):
        """One-call video step (demo.py:55-68 + 91-118): uint8 frames (N,H,W,3) or (H,W,3), numpy or cuda tensor -> upload,
        batched pre-processing, network, grouping and (if ``set_tracking`` is on) the pose tail, all enqueued; returns at once.
        Read the results with ``pipeline_fetch(slot)`` and ``poses(slot)`` (and, with ``set_overlay`` on, ``pipeline_overlay(slot)``).  The tail un-maps with this submit's own stride,
        scale and pad (``preprocess_dims`` of the frame size): ``set_unmap`` is neither used nor changed.  A numpy frame buffer
        may be reused on return; a cuda tensor is kept alive until the slot is fetched."""
        ptr, mem, N, H, W, a = self._u8_frames(frames)
        pv = (C.c_double * 3)(*[float(v) for v in pad_value])
        mv = (C.c_double * 3)(*[float(v) for v in img_mean])
        if mem == MEM_DEVICE:
            self._order(a.device)
        check(lib().lwp_pipeline_submit_u8(self.h.ptr, ptr, mem, N, H, W, net_input_height_size, stride, pv, mv, float(img_scale),
                                           upsample_ratio, 1 if demo else 0, slot), self.h.ptr)
        self._keep_slot = getattr(self, "_keep_slot", {})
        self._keep_slot[slot] = (a if mem == MEM_DEVICE else None, N)
        self._overlay_shape = getattr(self, "_overlay_shape", {})
        self._overlay_shape[slot] = (N, H, W, 3)

    def pipeline_fetch(self, slot):
        _, N = self._keep_slot[slot]
        counts, kpts, ent, ne, kcap, ecap = self._result_buffers(N)
        check(lib().lwp_pipeline_fetch(self.h.ptr, slot, counts.ctypes.data_as(C.POINTER(C.c_int)), kpts.ctypes.data, kcap,
                                       ent.ctypes.data, ecap, ne.ctypes.data_as(C.POINTER(C.c_int))), self.h.ptr)
        return self._unpack(N, counts, kpts, ent, ne)

    # ------------------------------------------------------------------ pose tail on the device (demo.py:101-118)
    TRACK_OFF, TRACK_ROWS, TRACK_LANES, TRACK_SEQUENCE = 0, 1, 2, 3

    def set_tracking(self, mode, match_threshold=3, similarity_threshold=0.5, smooth=False, sigmas=None):
        """Pose tail behind the grouping kernels: mode 0 off (default), 1 pose rows only, 2 lanes (frame f of a batch continues
        lane f), 3 sequence (the frames of a batch are consecutive frames of lane 0).  ``sigmas``: K float32 values as
        ``Pose.sigmas`` holds them; None = the COCO table (18 types only).  Clears every lane."""
        mode = {"off": 0, "rows": 1, "lanes": 2, "sequence": 3}.get(mode, mode)
        sg, n = None, 0
        if sigmas is not None:
            sg = np.ascontiguousarray(sigmas, dtype=np.float32)
            n = int(sg.size)
        check(lib().lwp_set_tracking(self.h.ptr, int(mode), int(match_threshold), float(similarity_threshold), 1 if smooth else 0,
                                     sg.ctypes.data_as(C.POINTER(C.c_float)) if sg is not None else None, n), self.h.ptr)
        self._tracking_mode = int(mode)

    def set_unmap(self, stride, scale, pad):
        """Geometry of the un-map (demo.py:101-103) for the following pose-producing calls; ``pad`` = [top, left, ...] as
        ``preprocess_dims`` / ``infer_fast`` return it."""
        check(lib().lwp_set_unmap(self.h.ptr, int(stride), float(scale), int(pad[0]), int(pad[1])), self.h.ptr)

    def reset_tracking(self, lane=-1, next_id=0):
        """Clears a lane (-1: all) and sets the first id it gives out."""
        check(lib().lwp_reset_tracking(self.h.ptr, int(lane), int(next_id)), self.h.ptr)

    def poses(self, slot=-1):
        """Pose rows of the last infer_poses / poses_from_maps / fetch_poses (slot -1) or of a fetched pipeline slot: per frame a
        dict of keypoints (P,K,2) int32, confidence (P,) f64, bbox (P,4) int32, ids (P,) int32 (-1 without tracking), last_id and
        near (similarity decisions the device could round differently from NumPy; 0 on every fixture)."""
        N = self._last_N if slot < 0 else self._keep_slot[slot][1]
        K, cap = self.skeleton["num_kpt_types"], self.caps[3]
        ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint)
        n = np.zeros(N, np.int32)
        kp = np.zeros((N, cap, K, 2), np.int32)
        conf = np.zeros((N, cap), np.float64)
        bbox = np.zeros((N, cap, 4), np.int32)
        ids = np.zeros((N, cap), np.int32)
        last = np.zeros(N, np.int32)
        near = np.zeros(N, np.uint32)
        check(lib().lwp_get_poses(self.h.ptr, slot, n.ctypes.data_as(ip), kp.ctypes.data_as(ip), conf.ctypes.data_as(C.POINTER(C.c_double)),
                                  bbox.ctypes.data_as(ip), ids.ctypes.data_as(ip), last.ctypes.data_as(ip), cap), self.h.ptr)
        check(lib().lwp_debug_tracking_near(self.h.ptr, slot, near.ctypes.data_as(up), N), self.h.ptr)
        return [dict(keypoints=kp[f, :n[f]].copy(), confidence=conf[f, :n[f]].copy(), bbox=bbox[f, :n[f]].copy(),
                     ids=ids[f, :n[f]].copy(), last_id=int(last[f]), near=int(near[f])) for f in range(N)]

    def track_poses_device(self, keypoints, confidence, lane=0):
        """One tracking step of ``lane`` on caller-supplied poses ((P,K,2) int32 key-points, (P,) confidences), on the kernels of
        the pose tail.  Returns dict(keypoints, bbox, ids, last_id, near)."""
        K = self.skeleton["num_kpt_types"]
        kp = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, K, 2)
        conf = np.ascontiguousarray(confidence, dtype=np.float64).reshape(-1)
        n = len(kp)
        if len(conf) != n:
            raise ValueError("%d poses but %d confidences" % (n, len(conf)))
        ip = C.POINTER(C.c_int)
        okp, obb, oid = np.zeros((n, K, 2), np.int32), np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
        last, near = C.c_int(), C.c_uint()
        check(lib().lwp_track_poses(self.h.ptr, int(lane), n, kp.ctypes.data_as(ip), conf.ctypes.data_as(C.POINTER(C.c_double)),
                                    okp.ctypes.data_as(ip), obb.ctypes.data_as(ip), oid.ctypes.data_as(ip), C.byref(last),
                                    C.byref(near)), self.h.ptr)
        return dict(keypoints=okp, bbox=obb, ids=oid, last_id=last.value, near=near.value)

    # ------------------------------------------------------------------ pose overlay on the device (demo.py:119-124)
    OVERLAY_OFF, OVERLAY_DEVICE, OVERLAY_HOST = 0, 1, 2

    def set_overlay(self, mode, color=None, box_color=None, boxes=True, n_draw_limbs=-1):
        """Skeletons, the 0.6 / 0.4 blend and the boxes of demo.py:119-124 drawn by kernels behind the pose tail of
        ``pipeline_submit_u8``: mode 0 off (default), 1 annotated frames kept on the device, 2 also copied to pinned host memory
        with the slot's results (``pipeline_overlay``).  ``color`` / ``box_color``: 3 bytes in the frame's channel order, None =
        ``Pose.color`` / (0, 255, 0); ``n_draw_limbs``: the first rows of the engine's limb table that are drawn, -1 = all but
        the last two.  Everything but the mode also applies to ``draw_poses``.  The id label (cv2.putText) is not drawn."""
        mode = {"off": 0, "device": 1, "host": 2}.get(mode, mode)

        def rgb(c):
            if c is None:
                return None
            v = [int(x) for x in c]
            if len(v) != 3 or min(v) < 0 or max(v) > 255:
                raise ValueError("a colour is 3 values in 0..255, got %r" % (c,))
            return (C.c_ubyte * 3)(*v)
        check(lib().lwp_set_overlay(self.h.ptr, int(mode), rgb(color), rgb(box_color), 1 if boxes else 0, int(n_draw_limbs)), self.h.ptr)
        self._overlay_mode = int(mode)

    def draw_poses(self, imgs, keypoints, bbox, n_poses=None, device_out=None):
        """The overlay kernels on poses the caller supplies.  ``imgs``: one frame (H,W,3) or a batch (N,H,W,3), uint8, numpy or
        a cuda tensor.  One frame: ``keypoints`` (P,K,2) and ``bbox`` (P,4) int32.  A batch: padded arrays (N,cap,K,2) / (N,cap,4)
        with ``n_poses`` (N,), or a list of N (P_f,K,2) arrays and a list of N (P_f,4) arrays.  Returns the annotated frames as a
        NEW array of the input's shape; ``imgs`` is not modified.  ``device_out``: None = the kind of ``imgs``, True = a cuda
        tensor, False = a numpy array."""
        torch = _torch()
        ptr, mem, N, H, W, a = self._u8_frames(imgs)
        single = len(a.shape) == 3
        K = self.skeleton["num_kpt_types"]
        if single or n_poses is None:
            kl = [keypoints] if single else list(keypoints)
            bl = [bbox] if single else list(bbox)
            if len(kl) != N or len(bl) != N:
                raise ValueError("%d frames but %d key-point arrays and %d box arrays" % (N, len(kl), len(bl)))
            kl = [np.asarray(k, dtype=np.int32).reshape(-1, K, 2) for k in kl]
            bl = [np.asarray(b, dtype=np.int32).reshape(-1, 4) for b in bl]
            for k, b in zip(kl, bl):
                if len(k) != len(b):
                    raise ValueError("%d poses but %d boxes" % (len(k), len(b)))
            n = np.array([len(k) for k in kl], np.int32)
            cap = int(n.max()) if N else 0
            kp = np.full((N, cap, K, 2), -1, np.int32)
            bb = np.zeros((N, cap, 4), np.int32)
            for f in range(N):
                kp[f, :n[f]] = kl[f]
                bb[f, :n[f]] = bl[f]
        else:
            kp = np.ascontiguousarray(keypoints, dtype=np.int32)
            bb = np.ascontiguousarray(bbox, dtype=np.int32)
            n = np.ascontiguousarray(n_poses, dtype=np.int32).reshape(-1)
            if kp.ndim != 4 or kp.shape[0] != N or kp.shape[2:] != (K, 2) or bb.shape != (N, kp.shape[1], 4) or n.shape != (N,):
                raise ValueError("expected keypoints (N,cap,%d,2), bbox (N,cap,4) and n_poses (N,) for %d frames" % (K, N))
            cap = int(kp.shape[1])
        on_dev = (mem == MEM_DEVICE) if device_out is None else bool(device_out)
        if on_dev:
            out = torch.empty(tuple(a.shape), dtype=torch.uint8, device=torch.device("cuda", self.device_id))
            optr, omem = out.data_ptr(), MEM_DEVICE
        else:
            out = np.empty(tuple(a.shape), np.uint8)
            optr, omem = out.ctypes.data, MEM_HOST
        if mem == MEM_DEVICE or omem == MEM_DEVICE:
            self._order()
        ip = C.POINTER(C.c_int)
        check(lib().lwp_draw_poses(self.h.ptr, ptr, mem, N, H, W, n.ctypes.data_as(ip), kp.ctypes.data_as(ip), bb.ctypes.data_as(ip),
                                   cap, optr, omem), self.h.ptr)
        return out

    def pipeline_overlay(self, slot, device=False):
        """The annotated frames (N,H,W,3) uint8 of a fetched slot that was submitted with the overlay on: a numpy array (from the
        pinned copy in mode 2), or with ``device=True`` a cuda tensor.  A new array each time."""
        torch = _torch()
        shape = self._overlay_shape[slot]
        if device:
            out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self.device_id))
            self._order()
            ptr, mem = out.data_ptr(), MEM_DEVICE
        else:
            out = np.empty(shape, np.uint8)
            ptr, mem = out.ctypes.data, MEM_HOST
        check(lib().lwp_get_overlay(self.h.ptr, slot, ptr, mem, shape[0], shape[1], shape[2]), self.h.ptr)
        return out

    # ------------------------------------------------------------------ training targets and loss (coco.py:48-61,71-159; loss.py)
    def train_targets(self, kpts, n_persons, image_hw, stride=8, sigma=7, paf_thickness=1, time_iters=0):
        """Key-point and PAF target maps rendered on the device.  ``kpts``: (N, Pmax, K, 3) float64 rows (x, y, visibility),
        numpy or a cuda tensor, persons in label order; ``n_persons``: (N,) counts; ``image_hw``: (H, W) of the frames.
        Returns float32 cuda tensors ``keypoint_maps`` (N, K + 1, H // stride, W // stride) and ``paf_maps`` (N, 2L, ...) for
        the engine's skeleton (``set_skeleton``; the default gives coco.py's channel layout).  With ``time_iters`` > 0 the
        kernel is launched that many times back to back and the call returns the milliseconds of all of them (HIP events)."""
        torch = _torch()
        H, W = int(image_hw[0]), int(image_hw[1])
        sk = self.skeleton
        K, L = sk["num_kpt_types"], len(sk["limb_kpts"])
        if getattr(kpts, "is_cuda", False):
            a = kpts.detach().to(torch.float64).contiguous()
            ptr, mem = a.data_ptr(), MEM_DEVICE
        else:
            a = np.ascontiguousarray(kpts, dtype=np.float64)
            ptr, mem = a.ctypes.data, MEM_HOST
        if len(a.shape) != 4 or tuple(a.shape[2:]) != (K, 3):
            raise ValueError("expected key-points of shape (N, Pmax, %d, 3), got %s" % (K, tuple(a.shape)))
        N, Pmax = int(a.shape[0]), int(a.shape[1])
        n = np.ascontiguousarray(n_persons, dtype=np.int32).reshape(-1)
        if n.shape != (N,):
            raise ValueError("expected %d person counts, got %s" % (N, n.shape))
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        dev = torch.device("cuda", self.device_id)
        kmaps = torch.empty((N, K + 1, H // stride, W // stride), dtype=torch.float32, device=dev)
        pmaps = torch.empty((N, 2 * L, H // stride, W // stride), dtype=torch.float32, device=dev)
        self._order()
        args = (self.h.ptr, ptr if Pmax else None, mem, n.ctypes.data_as(C.POINTER(C.c_int)), N, Pmax, H, W, stride, float(sigma),
                float(paf_thickness), kmaps.data_ptr(), pmaps.data_ptr())
        if time_iters:
            ms = C.c_float()
            check(lib().lwp_time_train_targets(*args, int(time_iters), C.byref(ms)), self.h.ptr)
            return ms.value
        check(lib().lwp_train_targets(*args), self.h.ptr)
        return kmaps, pmaps

    def mask_downsample(self, mask, stride=8):
        """(N, H, W) or (H, W) float32 mask (numpy or cuda tensor) -> the mean of each stride x stride block as a float32 cuda
        tensor (N, H // stride, W // stride): cv2.resize(mask, fx=fy=1/stride, INTER_AREA) of coco.py:48 where H and W are
        multiples of the stride (ValueError otherwise)."""
        torch = _torch()
        if getattr(mask, "is_cuda", False):
            a = mask.detach().to(torch.float32).contiguous()
            ptr, mem = a.data_ptr(), MEM_DEVICE
        else:
            a = np.ascontiguousarray(mask, dtype=np.float32)
            ptr, mem = a.ctypes.data, MEM_HOST
        single = len(a.shape) == 2
        if len(a.shape) not in (2, 3):
            raise ValueError("expected a mask of shape (N, H, W) or (H, W), got %s" % (tuple(a.shape),))
        N = 1 if single else int(a.shape[0])
        H, W = int(a.shape[-2]), int(a.shape[-1])
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        out = torch.empty((N, H // stride, W // stride), dtype=torch.float32, device=torch.device("cuda", self.device_id))
        self._order()
        check(lib().lwp_mask_downsample(self.h.ptr, ptr, mem, N, H, W, stride, out.data_ptr()), self.h.ptr)
        return out[0] if single else out

    # ------------------------------------------------------------------ training augmentation (datasets/transformations.py)
    def augment_batch(self, samples_or_plan, transforms=None, rng=None, stride=8, time_iters=0):
        """The pixels of a batch of augmented training samples in one kernel launch.  ``samples_or_plan``: a
        ``datasets.transformations.BatchPlan``, or the raw samples with ``transforms`` (and ``rng``) for ``plan_batch``.
        Sources may be NumPy arrays (packed, one upload for the batch) or cuda uint8 / float32 tensors (read in place).
        Returns four cuda tensors: ``image`` (N, 3, cy, cx) float32 = (pixel - 128) / 256, ``mask`` (N, cy, cx) uint8,
        ``mask_small`` (N, cy // stride, cx // stride) float32 (coco.py:48 on the uint8 mask) and ``kpts`` (N, Pmax, 18, 3)
        float64, the transformed key-points as ``train_targets`` takes them (person counts: the plan's ``n_persons``).  Where a
        sample carries ``"segmentations"`` (crowd RLE dicts) instead of a float mask, its mask is rendered on the device from the
        runs (``lwp_augment_batch_crowd``) and read in place; a batch without any takes ``lwp_augment_batch``.  With
        ``time_iters`` > 0 the kernels are launched that many times back to back and the call returns their milliseconds."""
        torch = _torch()
        from ._lib import AugmentPlan
        from .datasets.transformations import BatchPlan, plan_batch
        if not isinstance(samples_or_plan, BatchPlan) and transforms is None:
            raise ValueError("raw samples need the transforms to plan them with")
        plan = samples_or_plan if isinstance(samples_or_plan, BatchPlan) else plan_batch(samples_or_plan, transforms, rng)
        N = len(plan)
        cy, cx = plan.crop_hw
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be at least 1")
        dev = torch.device("cuda", self.device_id)
        recs = (AugmentPlan * N)()
        keep = []                                      # the arrays the records point into, alive until the call returns
        for n, g in enumerate(plan.records):
            img, msk = plan.images[n], plan.masks[n]
            on_device = getattr(img, "is_cuda", False)
            if msk is not None and getattr(msk, "is_cuda", False) != on_device:
                raise ValueError("sample %d: the image and its mask must both be host arrays or both cuda tensors" % n)
            if on_device:
                if img.dtype != torch.uint8 or (msk is not None and msk.dtype != torch.float32):
                    raise TypeError("sample %d: cuda sources must be a uint8 image and a float32 mask" % n)
                img = img.detach().contiguous()
                msk = None if msk is None else msk.detach().contiguous()
                ip, mp = img.data_ptr(), (None if msk is None else msk.data_ptr())
            else:
                if np.asarray(img).dtype != np.uint8:
                    raise TypeError("sample %d: the image must be uint8, got %s" % (n, np.asarray(img).dtype))
                img = np.ascontiguousarray(img, dtype=np.uint8)
                msk = None if msk is None else np.ascontiguousarray(msk, dtype=np.float32)
                ip, mp = img.ctypes.data, (None if msk is None else msk.ctypes.data)
            keep.append((img, msk))
            r = recs[n]
            r.image, r.mask, r.mem = ip, mp, (MEM_DEVICE if on_device else MEM_HOST)
            r.rs_scale = float(g["rs_scale"])
            for i in range(6):
                r.m[i] = float(g["minv"][i])
            r.src_h, r.src_w, r.rs_h, r.rs_w, r.area = g["src_h"], g["src_w"], g["rs_h"], g["rs_w"], int(g["area"])
            r.bound_h, r.bound_w, r.should_crop = g["bound_h"], g["bound_w"], int(g["should_crop"])
            r.dst_y0, r.dst_y1, r.dst_x0, r.dst_x1 = g["dst"]
            r.img_y0, r.img_x0 = g["src0"]
            r.flip = int(g["flip"])
            for c in range(3):
                r.warp_pad[c], r.crop_pad[c] = int(g["warp_pad"][c]), int(g["crop_pad"][c])
        image = torch.empty((N, 3, cy, cx), dtype=torch.float32, device=dev)
        mask = torch.empty((N, cy, cx), dtype=torch.uint8, device=dev)
        small = torch.empty((N, cy // stride, cx // stride), dtype=torch.float32, device=dev)
        self._order()
        args = (self.h.ptr, recs, N, cy, cx, stride, image.data_ptr(), mask.data_ptr(), small.data_ptr())
        if getattr(plan, "crowd_runs", None) is not None:
            if time_iters:
                raise ValueError("a batch with segmentations has no timing twin: time crowd_masks, and augment_batch without them")
            counts, seg_off, image_seg_off = plan.crowd_runs
            i64p = C.POINTER(C.c_int64)
            check(lib().lwp_augment_batch_crowd(*args[:6], counts.ctypes.data_as(i64p), seg_off.ctypes.data_as(i64p),
                                                image_seg_off.ctypes.data_as(i64p), *args[6:]), self.h.ptr)
            return image, mask, small, torch.from_numpy(plan.kpts).to(dev)
        if time_iters:
            ms = C.c_float()
            check(lib().lwp_time_augment_batch(*args, int(time_iters), C.byref(ms)), self.h.ptr)
            return ms.value
        check(lib().lwp_augment_batch(*args), self.h.ptr)
        return image, mask, small, torch.from_numpy(plan.kpts).to(dev)

    def crowd_masks(self, segmentations_per_image, sizes, time_iters=0):
        """``get_mask`` (coco.py:17-21) of all-ones masks for a batch, in one kernel launch.  ``segmentations_per_image``: per
        image a list of uncompressed RLE dicts (possibly empty); ``sizes``: per image (height, width).  Returns a list of
        (H, W) float32 cuda tensors, views of ONE buffer: 1 where no segmentation covers the pixel, 0 where any does.  With
        ``time_iters`` > 0 the kernel is launched that many times back to back and the call returns the milliseconds of all of
        them (HIP events)."""
        torch = _torch()
        from .datasets.coco import pack_crowd_runs
        sizes = [(int(h), int(w)) for h, w in sizes]
        counts, seg_off, image_seg_off = pack_crowd_runs(segmentations_per_image, sizes)
        N = len(sizes)
        heights = np.array([h for h, _ in sizes], dtype=np.int32)
        widths = np.array([w for _, w in sizes], dtype=np.int32)
        out_off = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(heights.astype(np.int64) * widths, out=out_off[1:])
        buf = torch.empty((max(int(out_off[-1]), 1),), dtype=torch.float32, device=torch.device("cuda", self.device_id))
        self._order()
        i64p, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int)
        args = (self.h.ptr, counts.ctypes.data_as(i64p), seg_off.ctypes.data_as(i64p), image_seg_off.ctypes.data_as(i64p),
                heights.ctypes.data_as(ip), widths.ctypes.data_as(ip), N, out_off.ctypes.data_as(i64p), buf.data_ptr())
        if time_iters:
            ms = C.c_float()
            check(lib().lwp_time_crowd_masks(*args, int(time_iters), C.byref(ms)), self.h.ptr)
            return ms.value
        check(lib().lwp_crowd_masks(*args), self.h.ptr)
        return [buf[int(out_off[n]):int(out_off[n + 1])].view(h, w) for n, (h, w) in enumerate(sizes)]

    # ------------------------------------------------------------------ JPEG files (cv2.imread's place)
    @staticmethod
    def jpeg_info(data):
        """The header of one baseline JPEG file (``bytes``): a dict of lwp_jpeg_header's fields (width, height, components,
        per-component sampling and quantisation table, restart interval, MCU and block counts, the Exif orientation or 0).
        Needs no GPU.  ValueError, naming the reason and the byte offset, for a file outside the scope (include/lwpose.h)."""
        data = bytes(data)
        hd = _lib.JpegHeader()
        check(lib().lwp_jpeg_info(data, len(data), C.byref(hd)))
        n = hd.components
        return {"width": hd.width, "height": hd.height, "components": n, "h_samp": list(hd.h_samp)[:n], "v_samp": list(hd.v_samp)[:n],
                "quant_table": list(hd.quant_table)[:n], "restart_interval": hd.restart_interval, "mcus_x": hd.mcus_x,
                "mcus_y": hd.mcus_y, "orientation": hd.orientation, "blocks_w": list(hd.blocks_w)[:n],
                "blocks_h": list(hd.blocks_h)[:n], "total_blocks": hd.total_blocks}

    @staticmethod
    def debug_jpeg_blocks(data):
        """The host half alone (tests; no GPU): (header dict, coefficients int16 (total_blocks, 64) in natural order and plane
        order, quantisation tables uint16 (4, 64) in natural order)."""
        data = bytes(data)
        hd = Engine.jpeg_info(data)
        coef = np.empty((hd["total_blocks"], 64), dtype=np.int16)
        qt = np.empty((4, 64), dtype=np.uint16)
        check(lib().lwp_debug_jpeg_blocks(data, len(data), coef.ctypes.data, coef.size, qt.ctypes.data))
        return hd, coef, qt

    def set_jpeg_entropy(self, mode, subseq_bytes=0):
        """Where ``decode_jpeg_batch`` decodes the Huffman data: ``"host"`` (the default) or ``"device"`` (the same
        pixels, refusals and messages).  ``subseq_bytes``: the bytes of a scan one lane owns, 0 (the default) or a multiple of 4
        from 4 to 1024.  ValueError for anything else."""
        if mode not in _lib.JPEG_ENTROPY_MODES:
            raise ValueError("entropy mode must be 'host' or 'device', not %r" % (mode,))
        check(lib().lwp_set_jpeg_entropy(self.h.ptr, _lib.JPEG_ENTROPY_MODES[mode], int(subseq_bytes)), self.h.ptr)
        self._jpeg_entropy, self._jpeg_subseq = mode, int(subseq_bytes)

    @staticmethod
    def _jpeg_args(files):
        N = len(files)
        data = (C.c_void_p * N)(*[C.cast(C.c_char_p(f), C.c_void_p) for f in files])
        lens = (C.c_size_t * N)(*[len(f) for f in files])
        return data, lens

    def debug_jpeg_entropy(self, files, subseq_bytes=0, time_iters=0):
        """The device entropy decoder alone (tests): ``[(status, coef or None, qtables or None)]`` per file, status 0 for an
        accepted file, whose coefficients and tables are laid out as ``debug_jpeg_blocks`` returns them; a refused file does not
        fail the call.  With ``time_iters`` > 0: (milliseconds of that many back-to-back runs of the kernels, the most sync rounds
        inside a workgroup, the most across workgroups)."""
        files = [bytes(f) for f in files]
        N = len(files)
        if N == 0:
            return []
        data, lens = self._jpeg_args(files)
        self._order()
        if time_iters:
            ms, rounds = C.c_float(), (C.c_int * 2)()
            check(lib().lwp_time_jpeg_entropy_batch(self.h.ptr, N, data, lens, int(subseq_bytes), int(time_iters), C.byref(ms), rounds), self.h.ptr)
            return ms.value, rounds[0], rounds[1]
        coefs, qts = [], []
        for f in files:
            hd = _lib.JpegHeader()
            blocks = 0 if lib().lwp_jpeg_info(f, len(f), C.byref(hd)) else hd.total_blocks
            coefs.append(np.zeros((max(blocks, 1), 64), dtype=np.int16))
            qts.append(np.zeros((4, 64), dtype=np.uint16))
        cp = (C.c_void_p * N)(*[c.ctypes.data for c in coefs])
        qp = (C.c_void_p * N)(*[q.ctypes.data for q in qts])
        status = (C.c_int * N)()
        check(lib().lwp_debug_jpeg_entropy_batch(self.h.ptr, N, data, lens, int(subseq_bytes), cp, qp, status), self.h.ptr)
        return [(int(status[i]), None, None) if status[i] else (0, coefs[i], qts[i]) for i in range(N)]

    @staticmethod
    def debug_jpeg_scan(data):
        """The host pre-pass of the device entropy decoder alone (tests; no GPU): a dict of ``status`` (0 accepted so far,
        1 refused, 2 too long for device mode), ``bytes`` (the un-stuffed scan), ``segments`` (uint32 (n, 4): byte offset, byte
        length, first MCU, MCU count), ``tables`` (the six flattened Huffman tables, uint8 (6, 1488)) and ``qtables`` (uint16
        (4, 64)).  ValueError if the header itself is refused."""
        data = bytes(data)
        hd = Engine.jpeg_info(data)
        n_mcus = hd["mcus_x"] * hd["mcus_y"]
        cap = -(-n_mcus // hd["restart_interval"]) if hd["restart_interval"] else 1
        out = np.zeros(len(data) + 8, dtype=np.uint8)
        segs = np.zeros((cap, 4), dtype=np.uint32)
        tables = np.zeros((6, 1488), dtype=np.uint8)
        qt = np.zeros((4, 64), dtype=np.uint16)
        nb, ns, status = C.c_size_t(), C.c_size_t(), C.c_int()
        check(lib().lwp_debug_jpeg_scan(data, len(data), out.ctypes.data, out.size, C.byref(nb), segs.ctypes.data, cap, C.byref(ns),
                                        tables.ctypes.data, qt.ctypes.data, C.byref(status)))
        return {"status": status.value, "bytes": out[:nb.value].tobytes(), "segments": segs[:ns.value].copy(), "tables": tables, "qtables": qt}

    def decode_jpeg_batch(self, files, time_iters=0, entropy=None):
        """``cv2.imread(.., IMREAD_COLOR)`` of a batch of baseline JPEG files (a list of ``bytes``), decoded in ONE device call:
        the Huffman data on the host, inverse DCT, up-sampling, colour conversion and the BGR store on the GPU, files of different
        sizes and samplings mixed.  Returns a list of cuda uint8 (H, W, 3) tensors, views of one allocation.  ValueError with the
        file's index for one outside the scope; nothing is written then.  The Exif orientation is not applied.  With
        ``time_iters`` > 0 each of the two kernels is launched that many times back to back and the call returns their
        milliseconds (stage A, stage B).  ``entropy``: ``"host"`` or ``"device"`` for this call, None for the engine's setting
        (``set_jpeg_entropy``; the host unless set)."""
        torch = _torch()
        if entropy is not None and entropy != getattr(self, "_jpeg_entropy", "host"):
            if entropy not in _lib.JPEG_ENTROPY_MODES:
                raise ValueError("entropy mode must be 'host' or 'device', not %r" % (entropy,))
            before = getattr(self, "_jpeg_entropy", "host")
            check(lib().lwp_set_jpeg_entropy(self.h.ptr, _lib.JPEG_ENTROPY_MODES[entropy], getattr(self, "_jpeg_subseq", 0)), self.h.ptr)
            try:
                return self.decode_jpeg_batch(files, time_iters)
            finally:
                check(lib().lwp_set_jpeg_entropy(self.h.ptr, _lib.JPEG_ENTROPY_MODES[before], getattr(self, "_jpeg_subseq", 0)), self.h.ptr)
        files = [bytes(f) for f in files]
        N = len(files)
        if N == 0:
            return []
        sizes = []
        for i, f in enumerate(files):
            hd = _lib.JpegHeader()
            rc = lib().lwp_jpeg_info(f, len(f), C.byref(hd))
            if rc:
                raise ValueError("image %d: %s" % (i, lib().lwp_last_error(None).decode("utf-8", "replace")))
            sizes.append((hd.height, hd.width))
        off = np.zeros(N + 1, dtype=np.int64)           # every image starts on a 16-byte boundary of the allocation
        for i, (h, w) in enumerate(sizes):
            off[i + 1] = (off[i] + h * w * 3 + 15) // 16 * 16
        buf = torch.empty((int(off[-1]),), dtype=torch.uint8, device=torch.device("cuda", self.device_id))
        data = (C.c_void_p * N)(*[C.cast(C.c_char_p(f), C.c_void_p) for f in files])
        lens = (C.c_size_t * N)(*[len(f) for f in files])
        outs = (C.c_void_p * N)(*[buf.data_ptr() + int(off[i]) for i in range(N)])
        self._order()
        if time_iters:
            ms = (C.c_float * 2)()
            check(lib().lwp_time_jpeg_decode_batch(self.h.ptr, N, data, lens, outs, int(time_iters), ms), self.h.ptr)
            return ms[0], ms[1]
        check(lib().lwp_jpeg_decode_batch(self.h.ptr, N, data, lens, outs), self.h.ptr)
        return [buf[int(off[i]):int(off[i]) + h * w * 3].view(h, w, 3) for i, (h, w) in enumerate(sizes)]

    def stage_losses(self, outs, keypoint_maps, paf_maps, mask, batch_size=None, time_iters=0):
        """train.py:92-97's per-stage sums: ``outs`` is the list net(x) returned (cuda tensors; an entry may be None),
        ``keypoint_maps`` / ``paf_maps`` the targets, ``mask`` one (N, h, w) cuda tensor broadcast over the channels.
        Returns 2 * (nref + 1) Python floats, loss[i] = sum(((outs[i] - target) * mask)**2 / 2 / batch_size) in float64;
        two calls on the same inputs return the same bits.  Tensors are read as contiguous NCHW float32: a strided view is
        copied first (``Engine.forward`` returns contiguous tensors, which are read in place).  With ``time_iters`` > 0 the
        kernels are launched that many times back to back and the call returns the milliseconds of all of them (HIP events)."""
        args, n = self._loss_args(outs, keypoint_maps, paf_maps, mask, batch_size)
        if time_iters:
            ms = C.c_float()
            check(lib().lwp_time_stage_losses(*args, int(time_iters), C.byref(ms)), self.h.ptr)
            return ms.value
        losses = (C.c_double * max(n, 1))()
        check(lib().lwp_stage_losses(*args, losses), self.h.ptr)
        return [float(losses[i]) for i in range(n)]

    def _loss_args(self, outs, keypoint_maps, paf_maps, mask, batch_size):
        """The leading arguments of lwp_stage_losses / lwp_stage_losses_log and the number of stage tensors; the contiguous
        tensors behind the pointers are kept on the engine until the next loss call."""
        torch = _torch()

        def dev32(t, what, shape):
            if t is None:
                return None
            if not getattr(t, "is_cuda", False):
                raise TypeError("%s must be a cuda tensor" % what)
            if tuple(t.shape) != shape:
                raise ValueError("%s has shape %s, expected %s" % (what, tuple(t.shape), shape))
            return t.detach().to(torch.float32).contiguous()
        ref = next((o for o in outs if o is not None), None)
        if ref is None:
            raise ValueError("no stage tensor given")
        N, _, hs, ws = (int(v) for v in ref.shape)
        keep = [dev32(o, "outs[%d]" % i, (N, self.NP if i % 2 else self.NH, hs, ws)) for i, o in enumerate(outs)]
        km = dev32(keypoint_maps, "keypoint_maps", (N, self.NH, hs, ws))
        pm = dev32(paf_maps, "paf_maps", (N, self.NP, hs, ws))
        m = dev32(mask, "mask", (N, hs, ws))
        if m is None:
            raise ValueError("mask is None")
        ptrs = (C.c_void_p * max(len(keep), 1))(*[None if o is None else o.data_ptr() for o in keep])
        self._loss_keep = (keep, km, pm, m, ptrs)
        self._order()
        return (self.h.ptr, ptrs, len(keep), None if km is None else km.data_ptr(), None if pm is None else pm.data_ptr(), m.data_ptr(),
                N, hs, ws, int(N if batch_size is None else batch_size)), len(keep)

    def log_stage_losses(self, outs, keypoint_maps, paf_maps, mask, batch_size=None, divisor=1.0):
        """``stage_losses`` without the read: the same launches, and behind them, on the device, ``log[i] += loss[i] / divisor``
        in float64 (train.py:96-97's total_losses with divisor = batches_per_iter).  Returns None and does not wait for the
        GPU; ``read_loss_log`` fetches the running sums.  ``divisor`` must be finite and > 0 (ValueError)."""
        args, _ = self._loss_args(outs, keypoint_maps, paf_maps, mask, batch_size)
        check(lib().lwp_stage_losses_log(*args, float(divisor)), self.h.ptr)

    def read_loss_log(self, reset=True):
        """(the 2 * (nref + 1) running sums of ``log_stage_losses`` as Python floats, the number of adds since the last reset).
        Waits for the engine's stream: the one wait of a logged training loop.  ``reset`` zeroes both behind the read."""
        S = 2 * (self.nref + 1)
        sums, adds = (C.c_double * S)(), C.c_int64()
        check(lib().lwp_loss_log_read(self.h.ptr, sums, C.byref(adds), 1 if reset else 0), self.h.ptr)
        return [float(sums[i]) for i in range(S)], int(adds.value)

    # ------------------------------------------------------------------ stage backward (train.py:99-103, fp32 engines)
    def train_forward(self, x):
        """``forward`` for a float32 cuda tensor (N, 3, H, W) that also keeps what ``stage_backward`` needs: every stage
        layer's output from cpm.conv on (from the cpm's input on in train scope "cpm", from model.0 on in scope "all").  Returns the same list of stage outputs, bit for bit."""
        torch = _torch()
        x = self._as_device_input(x)
        N, _, H, W = (int(v) for v in x.shape)
        fh, fw = H, W
        for _ in range(3):
            fh, fw = (fh - 1) // 2 + 1, (fw - 1) // 2 + 1
        outs = [torch.empty((N, self.NP if i % 2 else self.NH, fh, fw), dtype=torch.float32, device=x.device) for i in range(2 * (1 + self.nref))]
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        self._order(x.device)
        check(lib().lwp_train_forward(self.h.ptr, x.data_ptr(), N, H, W, ptrs), self.h.ptr)
        return outs

    def set_backward_precision(self, precision="fp32", grad_scale=1.0):
        """The operand type of the dense-conv gradients' two MFMA products: ``"fp32"`` (the default: the f32 kernels and their
        bits), ``"bf16"`` or ``"fp16"`` (include/lwpose.h, "backward precision").  dZ is multiplied by ``grad_scale``, a
        power of two in [1, 2^24] (1 with "fp32"), in front of its rounding and the f32 accumulator by its inverse.  Everything
        else, the engine included, stays fp32; the setting may change between any two calls.  ValueError for anything else."""
        if precision not in _lib.BACKWARD_PRECISIONS:
            raise ValueError("backward precision must be 'fp32', 'bf16' or 'fp16', not %r" % (precision,))
        check(lib().lwp_set_backward_precision(self.h.ptr, _lib.BACKWARD_PRECISIONS[precision], float(grad_scale)), self.h.ptr)

    @property
    def backward_precision(self):
        """(name, grad_scale) as the handle holds them."""
        dt, sc = C.c_int(), C.c_double()
        check(lib().lwp_get_backward_precision(self.h.ptr, C.byref(dt), C.byref(sc)), self.h.ptr)
        return [k for k, v in _lib.BACKWARD_PRECISIONS.items() if v == dt.value][0], sc.value

    def set_train_scope(self, scope):
        """"stages" (the default): ``train_forward`` / ``stage_backward`` / ``adam_step`` cover initial_stage.* and
        refinement_stages.*; "cpm": the cpm (cpm.align, cpm.trunk, cpm.conv) as well, its ten parameters in front of the stage
        ones in every flat array, the backbone frozen; "all": the backbone model.* too (its 69 parameters in front of the cpm's;
        BatchNorm at its running statistics, which never move).  Raises RuntimeError once the optimiser has taken a step
        (``load_adam_state(None)`` first, or set the scope before the first step).  The retained forward is invalidated.
        Parameters the old scope has trained and the new one does not cover stay readable through ``trained_params``."""
        name = _lib.train_scope_name(scope)
        if name == self.train_scope:
            check(lib().lwp_set_train_scope(self.h.ptr, _lib.train_scope(name)), self.h.ptr)
            return
        old = self.stage_params() if self.stage_steps != self._scope_steps else {}
        check(lib().lwp_set_train_scope(self.h.ptr, _lib.train_scope(name)), self.h.ptr)
        self.train_scope = name
        self._gspec = None
        self._scope_steps = self.stage_steps
        covered = set(k for k, _, _ in self.grad_spec()[0])
        self._left_params.update((k, v.clone()) for k, v in old.items() if k not in covered)
        for k in covered:
            self._left_params.pop(k, None)

    def grad_spec(self):
        """([(state-dict key, shape, float offset)], total floats) of the flat gradient array, in the engine's train scope."""
        if getattr(self, "_gspec", None) is None:
            self._gspec = _lib.train_grad_spec(self.train_scope, self.nref, self.C, self.NH, self.NP)
        return self._gspec

    def grad_views(self, flat):
        """dict key -> view of ``flat`` (the array ``stage_backward`` fills) with that parameter's shape."""
        return dict((k, flat[off:off + int(np.prod(shape))].view(shape)) for k, shape, off in self.grad_spec()[0])

    def _backward_args(self, keypoint_maps, paf_maps, mask, batch_size, loss_scale, flat, want_features):
        torch = _torch()
        if not getattr(mask, "is_cuda", False) or mask.dim() != 3:
            raise ValueError("mask must be an (N, h, w) cuda tensor")
        N, hs, ws = (int(v) for v in mask.shape)

        def dev32(t, what, shape):
            if not getattr(t, "is_cuda", False):
                raise TypeError("%s must be a cuda tensor" % what)
            if tuple(t.shape) != shape:
                raise ValueError("%s has shape %s, expected %s" % (what, tuple(t.shape), shape))
            return t.detach().to(torch.float32).contiguous()
        km = dev32(keypoint_maps, "keypoint_maps", (N, self.NH, hs, ws))
        pm = dev32(paf_maps, "paf_maps", (N, self.NP, hs, ws))
        m = dev32(mask, "mask", (N, hs, ws))
        dfeat = torch.empty((N, self.C, hs, ws), dtype=torch.float32, device=m.device) if want_features else None
        self._keep = (km, pm, m)
        return (self.h.ptr, km.data_ptr(), pm.data_ptr(), m.data_ptr(), N, hs, ws, int(N if batch_size is None else batch_size),
                float(loss_scale)), flat, dfeat

    def stage_backward(self, keypoint_maps, paf_maps, mask, batch_size=None, loss_scale=1.0, into=None, want_features=True, want_backbone=False):
        """Gradients of L = loss_scale * sum of the per-stage masked L2 losses (train.py:99-102) of the last ``train_forward``:
        returns (grads, d_features).  ``grads`` maps every initial_stage.* / refinement_stages.* state-dict key that has a
        gradient to a cuda tensor of the parameter's shape, all views of one flat array (``flat_of(grads)``); ``d_features`` is dL / d backbone_features (N, num_channels, h, w).  ``into``: a flat array from an
        earlier call (``Engine.flat_of(grads)``) to add to, like loss.backward() accumulates over train.py:96's batches.
        The refinement BatchNorms stay at their running statistics: the reference network in eval() mode.
        In train scope "cpm" the dict holds the cpm.* keys too, and ``want_backbone=True`` returns a third value: the gradient
        at the cpm's input (N, 512, h, w).  Train scope "all" adds the model.* keys; there is no gradient at the image."""
        torch = _torch()
        total = self.grad_spec()[1]
        dev = torch.device("cuda", self.device_id)
        if into is not None and (not into.is_cuda or into.dtype != torch.float32 or into.numel() != total or not into.is_contiguous()):
            raise ValueError("into must be the contiguous float32 cuda array of %d gradients an earlier call returned" % total)
        flat = into if into is not None else torch.empty(total, dtype=torch.float32, device=dev)
        args, flat, dfeat = self._backward_args(keypoint_maps, paf_maps, mask, batch_size, loss_scale, flat, want_features)
        self._order()
        if want_backbone:
            dback = torch.empty((dfeat.shape[0] if dfeat is not None else int(mask.shape[0]), 512) + tuple(int(v) for v in mask.shape[1:]),
                                dtype=torch.float32, device=dev)
            check(lib().lwp_train_backward(*args, 1 if into is not None else 0, flat.data_ptr(), None if dfeat is None else dfeat.data_ptr(),
                                           dback.data_ptr()), self.h.ptr)
            return self.grad_views(flat), dfeat, dback
        check(lib().lwp_stage_backward(*args, 1 if into is not None else 0, flat.data_ptr(), None if dfeat is None else dfeat.data_ptr()), self.h.ptr)
        return self.grad_views(flat), dfeat

    def flat_of(self, grads):
        """The flat array behind a dict ``stage_backward`` returned (to pass as ``into=``)."""
        flat = getattr(next(iter(grads.values())), "_base", None)
        if flat is None or flat.dim() != 1 or flat.numel() != self.grad_spec()[1]:
            raise ValueError("not a gradient dict of this engine's stage_backward")
        return flat

    def profile_stage_backward(self, keypoint_maps, paf_maps, mask, batch_size=None, loss_scale=1.0, reps=3):
        """Device milliseconds and launch counts of one backward by kernel class (HIP events around every launch)."""
        torch = _torch()
        flat = torch.empty(self.grad_spec()[1], dtype=torch.float32, device=torch.device("cuda", self.device_id))
        args, flat, dfeat = self._backward_args(keypoint_maps, paf_maps, mask, batch_size, loss_scale, flat, True)
        ms, n = (C.c_float * 4)(), (C.c_int * 4)()
        self._order()
        check(lib().lwp_profile_stage_backward(*args, flat.data_ptr(), dfeat.data_ptr(), int(reps), ms, n), self.h.ptr)
        names = ("elementwise", "dgrad", "wgrad", "reduce")
        return dict((names[i], dict(ms=float(ms[i]), launches=int(n[i]))) for i in range(4))

    def cpm_activations(self):
        """Train scope "cpm": the retained cpm tensors of the last ``train_forward`` as NCHW float32 numpy, by the oracle's tap
        names: "model.11" (the cpm's input), "cpm.align", "cpm.trunk.j.dw", "cpm.trunk.j" (pointwise output after ELU, in front
        of the residual add for j = 2), "cpm.sum" and "cpm" (tests)."""
        layers = self.layers()
        by = dict((i["name"], i["index"]) for i in layers)
        out = {"model.11": self.train_activation(by["cpm.align"] - 1), "cpm.align": self.train_activation(by["cpm.align"]),
               "cpm": self.train_activation(by["cpm.conv"])}
        for j in range(3):
            pw = by["cpm.trunk.%d.pw" % j]
            dw = by.get("cpm.trunk.%d.dw" % j)
            out["cpm.trunk.%d.dw" % j] = self.train_activation(dw) if dw is not None else self.train_activation(pw, _lib.KEPT_DEPTHWISE)
            out["cpm.trunk.%d" % j] = self.train_activation(pw, _lib.KEPT_NO_RESIDUAL if j == 2 else _lib.KEPT_OUTPUT)
        out["cpm.sum"] = self.train_activation(by["cpm.trunk.2.pw"])
        return out

    def train_activation(self, layer_index, which=_lib.KEPT_OUTPUT):
        """Retained output of a layer from the last ``train_forward`` as NCHW float32 numpy (tests): a stage layer or cpm.conv,
        in train scope "cpm" also a cpm layer or the backbone's last layer, in scope "all" any layer.  ``which``: ``_lib.KEPT_DEPTHWISE`` for the retained
        depthwise copy of a fused cpm trunk or backbone block (``cin`` channels), ``_lib.KEPT_NO_RESIDUAL`` for the block's output in
        front of its residual add."""
        info = self.layers()[layer_index]
        channels = info["cin"] if which == _lib.KEPT_DEPTHWISE else info["cout"]
        cap = 1 << 16
        dims = (C.c_int * 4)()
        while True:
            buf = np.empty(cap, np.float32)
            rc = lib().lwp_debug_train_copy(self.h.ptr, layer_index, which, buf.ctypes.data, buf.size, dims)
            if rc == _lib.LWP_ERR_ARG and lib().lwp_last_error(self.h.ptr) == b"dst too small" and cap < (1 << 31):
                cap *= 8
                continue
            check(rc, self.h.ptr)
            break
        n = dims[0] * dims[1] * dims[2] * dims[3]
        assert dims[1] == channels
        return buf[:n].reshape(dims[0], dims[1], dims[2], dims[3]).copy()

    def backbone_activations(self):
        """Train scope "all": the retained backbone tensors of the last ``train_forward`` as NCHW float32 numpy, by the oracle's
        tap names: "model.0", "model.i.dw" (a fused block's retained depthwise copy) and "model.i", i = 1..11 (tests)."""
        by = dict((i["name"], i["index"]) for i in self.layers())
        out = {"model.0": self.train_activation(by["model.0"])}
        for i in range(1, 12):
            pw = by["model.%d.pw" % i]
            dw = by.get("model.%d.dw" % i)
            out["model.%d.dw" % i] = self.train_activation(dw) if dw is not None else self.train_activation(pw, _lib.KEPT_DEPTHWISE)
            out["model.%d" % i] = self.train_activation(pw)
        return out

    def debug_dw_grad(self, dz, x, w, stride, dil, max_chunk=0):
        """The backbone's depthwise gradient kernels alone (tests): ``dz`` (N, C, Ho, Wo), ``x`` (N, C, H, W), ``w`` (C, 1, 3, 3)
        float32 cuda tensors -> (dx (N, C, H, W), G (C, 1, 3, 3), g (C,), pixel ranges taken)."""
        torch = _torch()
        N, Cn, H, W = (int(v) for v in x.shape)
        nhwc = lambda t: t.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        dzn, xn = nhwc(dz), nhwc(x)
        wt = w.detach().to(torch.float32).reshape(Cn, 9).t().contiguous()
        dx = torch.empty_like(xn)
        G = torch.empty((Cn, 1, 3, 3), dtype=torch.float32, device=xn.device)
        g = torch.empty(Cn, dtype=torch.float32, device=xn.device)
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_dw_grad_sd(self.h.ptr, dzn.data_ptr(), xn.data_ptr(), wt.data_ptr(), N, H, W, Cn, int(stride), int(dil), int(max_chunk),
                                         dx.data_ptr(), G.data_ptr(), g.data_ptr(), C.byref(splits)), self.h.ptr)
        return dx.permute(0, 3, 1, 2).contiguous(), G, g, splits.value

    def debug_stem_wgrad(self, dz, x, max_chunk=0):
        """The stem's weight gradient kernel alone (tests): ``dz`` (N, 32, Ho, Wo), ``x`` (N, 3, H, W) -> (G (32, 3, 3, 3), g (32,), ranges)."""
        torch = _torch()
        N, _, H, W = (int(v) for v in x.shape)
        dzn = dz.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        xc = x.detach().to(torch.float32).contiguous()
        G = torch.empty((32, 3, 3, 3), dtype=torch.float32, device=xc.device)
        g = torch.empty(32, dtype=torch.float32, device=xc.device)
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_stem_wgrad(self.h.ptr, dzn.data_ptr(), xc.data_ptr(), N, H, W, int(max_chunk), G.data_ptr(), g.data_ptr(), C.byref(splits)), self.h.ptr)
        return G, g, splits.value

    # ------------------------------------------------------------------ the stage and cpm gradient kernels alone (tests)
    # NCHW float32 cuda tensors in and out; the kernels see NHWC rows.  `fill` is what the rows hold outside the tensor's window
    # (padding channels, GUARD_ROWS rows behind the last pixel); the rows come back whole so that a test can look there.
    GUARD_ROWS = 3

    @staticmethod
    def _rows(t, ld=None, off=0, fill=0.0, guard=0):
        torch = _torch()
        N, Cn, H, W = (int(v) for v in t.shape)
        rows = torch.full((N * H * W + guard, Cn if ld is None else int(ld)), float(fill), dtype=torch.float32, device=t.device)
        rows[:N * H * W, off:off + Cn] = t.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(N * H * W, Cn)
        return rows

    @staticmethod
    def _nchw(rows, shape, off=0):
        N, Cn, H, W = (int(v) for v in shape)
        return rows[:N * H * W, off:off + Cn].reshape(N, H, W, Cn).permute(0, 3, 1, 2).contiguous()

    def debug_conv_grad(self, dz, x, w, dil=1, pad="graph", max_chunk=0, acc_from=None, no_bias=False, accumulate=False,
                        dx0=None, dw0=None, db0=None, windows=None, fill=0.0):
        """dgrad, wgrad and its reduction of a dense conv alone: ``dz`` (N, cout, H, W), ``x`` (N, cin, H, W), ``w`` (cout, cin, ks,
        ks); ``dx0`` / ``dw0`` / ``db0`` are what dx / dw / db hold before the call (default zeros); ``acc_from`` defaults to cin
        (overwrite); ``windows`` = ((dz_ld, dz_off), (x_ld, x_off), (dx_ld, dx_off)) puts the three tensors in wider rows.
        -> (dx (N, cin, H, W), dw, db, pixel ranges taken, the dx rows whole)."""
        torch = _torch()
        N, cin, H, W = (int(v) for v in x.shape)
        cout, ks = int(w.shape[0]), int(w.shape[2])
        (zl, zo), (xl, xo), (dl, do) = windows if windows is not None else ((cout, 0), (cin, 0), (cin, 0))
        dzr, xr = self._rows(dz, zl, zo, fill), self._rows(x, xl, xo, fill)
        dxr = self._rows(dx0 if dx0 is not None else torch.zeros_like(x), dl, do, fill, self.GUARD_ROWS)
        wc = w.detach().to(torch.float32).contiguous()
        dw = (dw0 if dw0 is not None else torch.zeros_like(wc)).detach().to(torch.float32).clone().contiguous()
        db = (db0 if db0 is not None else torch.zeros(cout, device=x.device)).detach().to(torch.float32).clone().contiguous()
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_conv_grad(self.h.ptr, dzr.data_ptr(), int(zl), int(zo), xr.data_ptr(), int(xl), int(xo), wc.data_ptr(), N, H, W, cout, cin,
                                        ks, int(dil), _lib.PAD_MODES[pad], int(max_chunk), cin if acc_from is None else int(acc_from),
                                        int(bool(no_bias)), int(bool(accumulate)), dxr.data_ptr(), int(dl), int(do), dw.data_ptr(), db.data_ptr(),
                                        C.byref(splits)), self.h.ptr)
        return self._nchw(dxr, x.shape, do), dw, db, splits.value, dxr

    def debug_cpm_dw_grad(self, dz, x, w, beta=False, accumulate=False, max_chunk=0, dx0=None, dw0=None, ld=None, fill=0.0):
        """The cpm's depthwise gradient kernels alone (stride 1, dilation 1): ``dz``, ``x`` (N, C, H, W), ``w`` (C, 1, 3, 3); ``ld``: the
        row stride of all three windows (default C).  -> (dx, dw (C, 1, 3, 3), pixel ranges taken, the dx rows whole)."""
        torch = _torch()
        N, Cn, H, W = (int(v) for v in x.shape)
        ld = Cn if ld is None else int(ld)
        dzr, xr = self._rows(dz, ld, 0, fill), self._rows(x, ld, 0, fill)
        dxr = self._rows(dx0 if dx0 is not None else torch.zeros_like(x), ld, 0, fill, self.GUARD_ROWS)
        wt = w.detach().to(torch.float32).reshape(Cn, 9).t().contiguous()
        dw = (dw0 if dw0 is not None else torch.zeros((Cn, 1, 3, 3), device=x.device)).detach().to(torch.float32).clone().contiguous()
        splits = C.c_int()
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_dw_grad(self.h.ptr, dzr.data_ptr(), ld, xr.data_ptr(), ld, wt.data_ptr(), N, H, W, Cn, int(bool(beta)),
                                      int(bool(accumulate)), int(max_chunk), dxr.data_ptr(), ld, dw.data_ptr(), C.byref(splits)), self.h.ptr)
        return self._nchw(dxr, x.shape), dw, splits.value, dxr

    def debug_loss_grad(self, outs, keypoint_maps, paf_maps, mask, scale, ld=None, off=0, fill=0.0):
        """``loss_grad_kernel`` alone: ``outs`` alternate (N, CH, h, w) and (N, CP, h, w) tensors, ``mask`` (N, h, w), ``scale`` the
        float32 factor loss_scale / batch.  -> ([gradient like outs[s]], [its rows whole])."""
        torch = _torch()
        N, CH, hh, ww = (int(v) for v in keypoint_maps.shape)
        CP = int(paf_maps.shape[1])
        ld = off + max(CH, CP) if ld is None else int(ld)
        S = len(outs)
        src = [self._rows(o, ld, off, fill) for o in outs]
        dst = [self._rows(torch.zeros_like(o), ld, off, fill, self.GUARD_ROWS) for o in outs]
        vp = C.c_void_p
        a = (vp * S)(*[t.data_ptr() + 4 * off for t in src])
        b = (vp * S)(*[t.data_ptr() + 4 * off for t in dst])
        km, pm, mk = (t.detach().to(torch.float32).contiguous() for t in (keypoint_maps, paf_maps, mask))
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_loss_grad(self.h.ptr, a, b, S, ld, km.data_ptr(), pm.data_ptr(), mk.data_ptr(), N, CH, CP, hh * ww, float(scale)), self.h.ptr)
        return [self._nchw(d, o.shape, off) for d, o in zip(dst, outs)], dst

    def _debug_rows_op(self, call, g, others, ld, fill):
        torch = _torch()
        N, Cn, H, W = (int(v) for v in g.shape)
        ld = Cn if ld is None else int(ld)
        gr = self._rows(g, ld, 0, fill, self.GUARD_ROWS)
        rs = [self._rows(o, ld, 0, fill) if o is not None else None for o in others]
        self._order()
        torch.cuda.synchronize()
        check(call(gr, rs, ld, N * H * W, Cn), self.h.ptr)
        return self._nchw(gr, g.shape), gr

    def debug_relu_mask(self, g, y, res=None, ld=None, fill=0.0):
        """g where y > res (``res`` None: y > 0), else 0; all (N, C, H, W).  -> (result, its rows whole)."""
        return self._debug_rows_op(lambda gr, rs, ld, M, Cn: lib().lwp_debug_relu_mask(
            self.h.ptr, gr.data_ptr(), ld, rs[0].data_ptr(), ld, rs[1].data_ptr() if rs[1] is not None else None, ld, M, Cn), g, [y, res], ld, fill)

    def debug_grad_add(self, dst, src, beta, ld=None, fill=0.0):
        """(beta ? dst : 0) + src.  -> (result, its rows whole)."""
        return self._debug_rows_op(lambda gr, rs, ld, M, Cn: lib().lwp_debug_grad_add(
            self.h.ptr, gr.data_ptr(), ld, rs[0].data_ptr(), ld, M, Cn, int(bool(beta))), dst, [src], ld, fill)

    def debug_elu_grad(self, g, y, ld=None, fill=0.0):
        """g * (y > 0 ? 1 : y + 1), y the ELU's output.  -> (result, its rows whole)."""
        return self._debug_rows_op(lambda gr, rs, ld, M, Cn: lib().lwp_debug_elu_grad(
            self.h.ptr, gr.data_ptr(), ld, rs[0].data_ptr(), ld, M, Cn), g, [y], ld, fill)

    def debug_pw_fold(self, w, gamma, var):
        """``pw_fold_kernel`` alone: ``w`` (cout, cin), ``gamma`` and ``var`` (cout,) -> the folded (cout, cin) matrix."""
        torch = _torch()
        w, gamma, var = (t.detach().to(torch.float32).contiguous() for t in (w, gamma, var))
        out = torch.empty_like(w)
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_pw_fold(self.h.ptr, w.data_ptr(), gamma.data_ptr(), var.data_ptr(), out.data_ptr(), int(w.shape[0]), int(w.shape[1])), self.h.ptr)
        return out

    def debug_bn_chain(self, G, g, W, b, gamma, mean, var, into, accumulate=False):
        """``bn_chain_kernel`` alone: ``G`` and ``W`` (cout, K), the others (cout,); ``into`` = (dW, db or None, dgamma, dbeta), contiguous
        float32 cuda arrays written in place (they may be views into wider arrays)."""
        torch = _torch()
        ins = [t.detach().to(torch.float32).contiguous() for t in (G, g, W, b, gamma, mean, var)]
        for t in into:
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("outputs must be contiguous float32 cuda arrays")
        self._order()
        torch.cuda.synchronize()
        check(lib().lwp_debug_bn_chain(self.h.ptr, *([t.data_ptr() for t in ins] + [t.data_ptr() if t is not None else None for t in into]
                                                    + [int(ins[0].shape[0]), int(ins[0].shape[1]), int(bool(accumulate))])), self.h.ptr)

    def backward_splits(self, layer_index, depthwise=False):
        """Pixel ranges the last ``stage_backward`` split this layer's weight gradient into (0: none ran); ``depthwise``: those
        of the layer's depthwise weight gradient (a depthwise layer or a fused block of the cpm trunk, train scope "cpm")."""
        n = (lib().lwp_debug_backward_dw_splits if depthwise else lib().lwp_debug_backward_splits)(self.h.ptr, layer_index)
        if n < 0:
            raise ValueError("bad layer index")
        return n

    # ------------------------------------------------------------------ stage fine-tuning step (train.py:41-55, :106; fp32 engines)
    def _flat32(self, flat, what):
        torch = _torch()
        total = self.grad_spec()[1]
        if not getattr(flat, "is_cuda", False) or flat.dtype != torch.float32 or flat.numel() != total or not flat.is_contiguous():
            raise ValueError("%s must be a contiguous float32 cuda array of %d values in the gradient-spec layout" % (what, total))
        return flat

    def adam_groups(self):
        """[(state-dict key, learning-rate multiplier, weight decay on)] per gradient-spec entry (train.py:41-55)."""
        return _lib.train_adam_groups(self.train_scope, self.nref, self.C, self.NH, self.NP)

    def adam_step(self, flat, base_lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4):
        """One step of the reference's Adam (its parameter groups included) on the stage parameters from the flat gradient array
        ``stage_backward`` filled (``flat_of(grads)``), then the device-side refold and repack of the stage layers: the engine
        is afterwards as if ``load_state_dict`` had been called with the new values, with no host copy and no synchronise.
        The retained ``train_forward`` is invalidated."""
        flat = self._flat32(flat, "flat")
        self._order()
        check(lib().lwp_stage_adam_step(self.h.ptr, flat.data_ptr(), float(base_lr), float(betas[0]), float(betas[1]), float(eps),
                                        float(weight_decay)), self.h.ptr)
        self.stage_steps += 1

    def stage_params(self):
        """dict state-dict key -> current raw stage parameter (float32 cuda tensors, views of one flat array in the
        gradient-spec layout: ``flat_of`` gives it)."""
        torch = _torch()
        flat = torch.empty(self.grad_spec()[1], dtype=torch.float32, device=torch.device("cuda", self.device_id))
        self._order()
        check(lib().lwp_stage_params_get(self.h.ptr, flat.data_ptr()), self.h.ptr)
        return self.grad_views(flat)

    def trained_params(self):
        """``stage_params`` plus what an earlier, wider train scope trained and the current one no longer covers (the cpm.*
        parameters after "cpm" -> "stages", the model.* ones after "all" -> "cpm"): every parameter whose value on the device may differ from what was loaded."""
        out = dict(self._left_params)
        out.update(self.stage_params())
        return out

    def adam_state(self):
        """dict(step, exp_avg, exp_avg_sq): the step count and the two flat float32 cuda arrays (gradient-spec layout)."""
        torch = _torch()
        dev = torch.device("cuda", self.device_id)
        m = torch.empty(self.grad_spec()[1], dtype=torch.float32, device=dev)
        v = torch.empty_like(m)
        step = C.c_int64()
        self._order()
        check(lib().lwp_stage_adam_state_get(self.h.ptr, m.data_ptr(), v.data_ptr(), C.byref(step)), self.h.ptr)
        return dict(step=int(step.value), exp_avg=m, exp_avg_sq=v)

    def load_adam_state(self, state):
        """Restores what ``adam_state`` returned (arrays on the host or the device); ``None`` discards the state."""
        if state is None:
            check(lib().lwp_stage_adam_reset(self.h.ptr), self.h.ptr)
            return
        torch = _torch()
        dev = torch.device("cuda", self.device_id)
        m = self._flat32(torch.as_tensor(state["exp_avg"]).to(dev, torch.float32).contiguous(), "exp_avg")
        v = self._flat32(torch.as_tensor(state["exp_avg_sq"]).to(dev, torch.float32).contiguous(), "exp_avg_sq")
        self._order()
        check(lib().lwp_stage_adam_state_set(self.h.ptr, m.data_ptr(), v.data_ptr(), int(state["step"])), self.h.ptr)

    def time_adam_step(self, flat, base_lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, iters=20):
        """(ms of ``iters`` Adam-kernel launches, ms of ``iters`` repack launches) on scratch copies (HIP events)."""
        flat = self._flat32(flat, "flat")
        ms = (C.c_float * 2)()
        self._order()
        check(lib().lwp_time_stage_adam_step(self.h.ptr, flat.data_ptr(), float(base_lr), float(betas[0]), float(betas[1]), float(eps),
                                             float(weight_decay), int(iters), ms), self.h.ptr)
        return float(ms[0]), float(ms[1])

    # ------------------------------------------------------------------ measurement
    def time_pipeline(self, x_cuda, iters, what=1, upsample_ratio=4, demo=True):
        """milliseconds for ``iters`` back-to-back passes (HIP events on the engine's stream)."""
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        ms = C.c_float()
        check(lib().lwp_time_pipeline(self.h.ptr, x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, what, iters, C.byref(ms)), self.h.ptr)
        self._last_N = N
        return ms.value

    def time_layer(self, layer_index, N, H, W, iters=50):
        ms = C.c_float()
        check(lib().lwp_debug_time_layer(self.h.ptr, layer_index, N, H, W, iters, C.byref(ms)), self.h.ptr)
        return ms.value

    def profile_launches(self, x_cuda, reps=5, upsample_ratio=4, demo=True):
        """[(name, class, ms)] per launch in issue order (HIP events around every launch)."""
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        cap = 256
        ms = (C.c_float * cap)()
        kc = (C.c_int * cap)()
        n = C.c_int()
        check(lib().lwp_profile_launches(self.h.ptr, x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, reps, ms, kc, cap, C.byref(n)), self.h.ptr)
        layers = self.layers()
        post = ["find_peaks", "nms", "score_pairs", "match", "assemble", "tail_rows", "tail_track"]
        out, npost = [], 0
        for i in range(n.value):
            li = (kc[i] >> 8) - 1                      # first layer the launch covers (a fused head pair is one launch), -1: post kernel
            if li >= 0:
                name = layers[li]["name"]
            else:
                name = post[npost] if npost < len(post) else "launch%d" % i
                npost += 1
            out.append((name, kc[i] & 0xff, ms[i]))
        return out

    def profile_classes(self, x_cuda, reps=5, upsample_ratio=4, demo=True):
        x_cuda = self._as_device_input(x_cuda)
        N, _, H, W = x_cuda.shape
        ms = (C.c_float * 6)()
        ln = (C.c_int * 6)()
        check(lib().lwp_profile_classes(self.h.ptr, x_cuda.data_ptr(), N, H, W, upsample_ratio, 1 if demo else 0, reps, ms, ln), self.h.ptr)
        names = ["stem", "depthwise", "pointwise_1x1", "dense_3x3", "post", "other"]
        return {n: {"ms": ms[i], "launches": ln[i]} for i, n in enumerate(names)}


    # ------------------------------------------------------------------ COCO key-point evaluation (val.py:17-27)
    @staticmethod
    def _coco_args(packed):
        i64p, dp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int)

        def ptr(a, t):
            return a.ctypes.data_as(t) if a.size else None
        return (int(packed["n_images"]), packed["dt_off"].ctypes.data_as(i64p), ptr(packed["dt_kp"], dp), ptr(packed["dt_score"], dp),
                packed["gt_off"].ctypes.data_as(i64p), ptr(packed["gt_kp"], dp), ptr(packed["gt_area"], dp), ptr(packed["gt_bbox"], dp),
                ptr(packed["gt_iscrowd"], ip), ptr(packed["gt_ignore"], ip))

    @staticmethod
    def _coco_gt_args(packed):
        """n_images and the ground-truth pointers of ``_coco_args``: what lwp_coco_open takes."""
        i64p, dp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int)

        def ptr(a, t):
            return a.ctypes.data_as(t) if a.size else None
        return (int(packed["n_images"]), packed["gt_off"].ctypes.data_as(i64p), ptr(packed["gt_kp"], dp), ptr(packed["gt_area"], dp),
                ptr(packed["gt_bbox"], dp), ptr(packed["gt_iscrowd"], ip), ptr(packed["gt_ignore"], ip))

    def coco_eval(self, gt, detections=None):
        """COCOeval(gt, loadRes(detections), 'keypoints') evaluate() + accumulate() on the GPU with COCOeval's default
        parameters.  ``gt``: a COCO ground-truth dict ('images', 'annotations', 'categories') with ``detections`` the list of
        result dicts (``val.coco_detections``), or the arrays ``coco_pack`` made of the two.  Returns a dict: ``precision``
        (10, 101, 3) and ``scores`` (10, 101, 3) indexed [IoU threshold, recall threshold, area range], ``recall`` (10, 3),
        ``npig`` (3,) and ``stats``, the ten numbers of summarize().  Two calls on the same input return the same bits."""
        packed = gt if detections is None and "dt_off" in gt else coco_pack(gt, detections)
        precision = np.empty((10, 101, 3), dtype=np.float64)
        scores = np.empty((10, 101, 3), dtype=np.float64)
        recall = np.empty((10, 3), dtype=np.float64)
        npig = np.zeros(3, dtype=np.int64)
        dp = C.POINTER(C.c_double)
        check(lib().lwp_coco_eval(self.h.ptr, *self._coco_args(packed), precision.ctypes.data_as(dp), recall.ctypes.data_as(dp),
                                  scores.ctypes.data_as(dp), npig.ctypes.data_as(C.POINTER(C.c_int64))), self.h.ptr)
        return {"precision": precision, "recall": recall, "scores": scores, "npig": npig, "stats": coco_stats(precision, recall)}

    def debug_coco_oks(self, gt, detections=None, image=0):
        """The per-image half of ``coco_eval`` for image number ``image`` (position in ascending image-id order): ``order``, the
        indices within the image of its up to 20 selected detections by rank; ``oks`` (len(order), G), columns in the ground
        truths' input order; ``matched`` / ``ignored`` (3, 10, 20) bool by [area range, IoU threshold, rank]; ``npig`` (3,)."""
        packed = gt if detections is None and "dt_off" in gt else coco_pack(gt, detections)
        image = int(image)
        if not 0 <= image < int(packed["n_images"]):
            raise ValueError("image %d out of range" % image)
        G = int(packed["gt_off"][image + 1] - packed["gt_off"][image])
        n_sel, order, npig = C.c_int(), (C.c_int * 20)(), (C.c_int * 3)()
        oks = np.zeros((20, max(G, 1)), dtype=np.float64)
        matched, ignored = np.zeros((30, 20), dtype=np.uint8), np.zeros((30, 20), dtype=np.uint8)
        ubp = C.POINTER(C.c_ubyte)
        check(lib().lwp_debug_coco_oks(self.h.ptr, *self._coco_args(packed), image, C.byref(n_sel), order, oks.ctypes.data_as(C.POINTER(C.c_double)),
                                       oks.size, matched.ctypes.data_as(ubp), ignored.ctypes.data_as(ubp), npig), self.h.ptr)
        n = n_sel.value
        return {"order": [order[r] for r in range(n)], "oks": oks.reshape(-1)[:n * G].reshape(n, G).copy(),
                "matched": matched.reshape(3, 10, 20).astype(bool), "ignored": ignored.reshape(3, 10, 20).astype(bool),
                "npig": np.array([npig[a] for a in range(3)], dtype=np.int64)}

    # ------------------------------------------------------------------ device-resident validation (val.py:113-160)
    def coco_open(self, gt_or_packed, row_cap=None):
        """Upload a data set's ground truth once and open a detection store of ``row_cap`` rows on the device (default: 32 an
        image).  ``gt_or_packed``: a COCO ground-truth dict, or what ``coco_pack_gt`` / ``coco_pack`` made of one.  A second
        call replaces the store.  Returns the packed ground truth (``image_ids`` gives an image's index)."""
        g = gt_or_packed if "gt_off" in gt_or_packed else coco_pack_gt(gt_or_packed)
        n = int(g["n_images"])
        row_cap = 32 * n if row_cap is None else int(row_cap)
        check(lib().lwp_coco_open(self.h.ptr, *self._coco_gt_args(g), row_cap), self.h.ptr)
        self._coco_n = n
        self._val_store = None                # (val.evaluate(store=True) notes here which labels the store belongs to)
        return g

    def coco_release(self):
        self._val_store = None
        check(lib().lwp_coco_release(self.h.ptr), self.h.ptr)

    def coco_reset(self):
        """Forget the detections and the status, keep the ground truth: the next validation of the same data set."""
        check(lib().lwp_coco_reset(self.h.ptr), self.h.ptr)

    def coco_add_maps(self, heat, paf, image_index, upsample_ratio=4, demo=False, layout="NCHW"):
        """``poses_from_maps`` for cuda tensors whose poses go into the detection store instead of to the host: grouping and the
        append kernel are enqueued and the call returns; nothing is synchronised or fetched.  ``image_index``: per frame its
        image's position in the ground truth's ascending id order."""
        lay = {"NCHW": 0, "NHWC": 1}[layout]
        if not getattr(heat, "is_cuda", False) or not getattr(paf, "is_cuda", False):
            raise TypeError("coco_add_maps takes cuda tensors (the maps stay on the device)")
        heat, paf = heat.detach().contiguous(), paf.detach().contiguous()
        if lay == 0:
            N, _, hs, ws = heat.shape
        else:
            N, hs, ws, _ = heat.shape
        idx = np.ascontiguousarray(np.atleast_1d(image_index), dtype=np.int32)
        if idx.shape != (N,):
            raise ValueError("image_index must hold one index per frame (%d), got %s" % (N, idx.shape))
        self._order(heat.device)
        check(lib().lwp_coco_add_maps(self.h.ptr, heat.data_ptr(), paf.data_ptr(), lay, N, hs, ws, upsample_ratio, 1 if demo else 0,
                                      idx.ctypes.data_as(C.POINTER(C.c_int))), self.h.ptr)

    def coco_add_rows(self, image_index, keypoints, scores):
        """Append ready-made detections of one image: ``keypoints`` (n, 17, 3) or (n, 51), ``scores`` (n,); enqueue only."""
        kp = np.ascontiguousarray(keypoints, dtype=np.float64).reshape(-1, 17, 3)
        sc = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
        if len(kp) != len(sc):
            raise ValueError("%d key-point rows but %d scores" % (len(kp), len(sc)))
        dp = C.POINTER(C.c_double)
        check(lib().lwp_coco_add_rows(self.h.ptr, int(image_index), len(sc), kp.ctypes.data_as(dp) if len(sc) else None,
                                      sc.ctypes.data_as(dp) if len(sc) else None), self.h.ptr)

    def coco_counts(self):
        """(rows in the store, rows per image (n_images,) int32) after everything queued so far; raises the store's status."""
        total = C.c_int64()
        per = np.zeros(self._coco_n, dtype=np.int32)
        check(lib().lwp_coco_counts(self.h.ptr, C.byref(total), per.ctypes.data_as(C.POINTER(C.c_int))), self.h.ptr)
        return int(total.value), per

    def coco_rows(self):
        """The store's rows in the evaluation's order (images ascending, within an image as added): ``image`` (n,) int32,
        ``keypoints`` (n, 17, 3) and ``score`` (n,) float64.  Two library calls, one synchronise each: ``coco_counts`` sizes
        the arrays (sizing them by the store's capacity instead would copy every unused row back), lwp_coco_rows fills them."""
        n, _ = self.coco_counts()
        img = np.zeros(n, dtype=np.int32)
        kp = np.zeros((n, 17, 3), dtype=np.float64)
        sc = np.zeros(n, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(lib().lwp_coco_rows(self.h.ptr, img.ctypes.data_as(C.POINTER(C.c_int)), kp.ctypes.data_as(dp), sc.ctypes.data_as(dp), n), self.h.ptr)
        return {"image": img, "keypoints": kp, "score": sc}

    def coco_finish(self):
        """``coco_eval`` on the store's rows against the resident ground truth: the same dict, bit for bit what ``coco_eval``
        returns for the same rows.  The store stays as it is."""
        precision = np.empty((10, 101, 3), dtype=np.float64)
        scores = np.empty((10, 101, 3), dtype=np.float64)
        recall = np.empty((10, 3), dtype=np.float64)
        npig = np.zeros(3, dtype=np.int64)
        dp = C.POINTER(C.c_double)
        check(lib().lwp_coco_finish(self.h.ptr, precision.ctypes.data_as(dp), recall.ctypes.data_as(dp), scores.ctypes.data_as(dp),
                                    npig.ctypes.data_as(C.POINTER(C.c_int64))), self.h.ptr)
        return {"precision": precision, "recall": recall, "scores": scores, "npig": npig, "stats": coco_stats(precision, recall)}

    def debug_coco_rows(self, frames, image_index):
        """The append kernel alone: ``frames`` is a list of (pose_entries (P, 20), all_keypoints (n, 4)) as ``poses_from_maps``
        returns them, loaded into the serial result block and appended as images ``image_index``."""
        N = len(frames)
        ne = np.array([len(f[0]) for f in frames], dtype=np.int32)
        nk = np.array([len(f[1]) for f in frames], dtype=np.int32)
        ent = np.ascontiguousarray(np.concatenate([np.asarray(f[0], dtype=np.float64).reshape(-1, 20) for f in frames]))
        kpt = np.ascontiguousarray(np.concatenate([np.asarray(f[1], dtype=np.float64).reshape(-1, 4) for f in frames]))
        idx = np.ascontiguousarray(image_index, dtype=np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        check(lib().lwp_debug_coco_rows(self.h.ptr, N, ent.ctypes.data_as(dp) if ent.size else None, ne.ctypes.data_as(ip),
                                        kpt.ctypes.data_as(dp) if kpt.size else None, nk.ctypes.data_as(ip), idx.ctypes.data_as(ip)), self.h.ptr)


def coco_pack(gt, detections):
    """The arrays ``lwp_coco_eval`` takes, from a COCO ground-truth dict and a list of result dicts, as COCO() / loadRes() /
    COCOeval._prepare() arrange them: the images of ``gt`` in ascending id order, each with its annotations and detections in
    input order; ``gt_ignore`` = iscrowd or num_keypoints == 0.  ValueError: a detection whose image_id is not in ``gt``
    (loadRes asserts this), a non-positive annotation id (COCOeval reads a match to id 0 as no match), more than one category."""
    g, index, cat = _coco_gt(gt)
    n = g["n_images"]
    per_dt = [[] for _ in range(n)]
    for d in detections:
        if int(d["image_id"]) not in index:
            raise ValueError("detection for image %r, which the ground truth does not list" % (d["image_id"],))
        if cat is not None and int(d.get("category_id", cat)) != cat:
            continue
        per_dt[index[int(d["image_id"])]].append(d)
    dts = [d for lst in per_dt for d in lst]
    return {"n_images": n, "image_ids": g["image_ids"],
            "dt_off": np.cumsum([0] + [len(v) for v in per_dt], dtype=np.int64), "dt_kp": _coco_kp(dts),
            "dt_score": np.array([d["score"] for d in dts], dtype=np.float64),
            "gt_off": g["gt_off"], "gt_kp": g["gt_kp"], "gt_area": g["gt_area"], "gt_bbox": g["gt_bbox"],
            "gt_iscrowd": g["gt_iscrowd"], "gt_ignore": g["gt_ignore"]}


def _coco_kp(rows):
    a = np.array([r["keypoints"] for r in rows], dtype=np.float64).reshape(-1, 17, 3) if rows else np.zeros((0, 17, 3))
    return np.ascontiguousarray(a)


def _coco_gt(gt):
    """(the ground-truth arrays, image id -> position, the one category id or None): the half of ``coco_pack`` that does not
    change while a data set is validated again and again."""
    cats = sorted({int(c["id"]) for c in gt["categories"]}) if gt.get("categories") else \
        sorted({int(a["category_id"]) for a in gt.get("annotations", []) if "category_id" in a})
    if len(cats) > 1:
        raise ValueError("COCO evaluation supports one category, the ground truth has %d" % len(cats))
    cat = cats[0] if cats else None
    img_ids = sorted({int(im["id"]) for im in gt["images"]})
    index = {v: i for i, v in enumerate(img_ids)}
    n = len(img_ids)
    if n < 1:
        raise ValueError("the ground truth lists no image")
    per_gt = [[] for _ in range(n)]
    for a in gt.get("annotations", []):
        if int(a["id"]) <= 0:
            raise ValueError("annotation id %r is not positive" % (a["id"],))
        if cat is not None and int(a.get("category_id", cat)) != cat:
            continue
        if int(a["image_id"]) in index:
            per_gt[index[int(a["image_id"])]].append(a)
    gts = [a for lst in per_gt for a in lst]
    crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in gts], dtype=np.int32)
    nokp = np.array([1 if a["num_keypoints"] == 0 else 0 for a in gts], dtype=np.int32)
    return ({"n_images": n, "image_ids": img_ids,
             "gt_off": np.cumsum([0] + [len(v) for v in per_gt], dtype=np.int64), "gt_kp": _coco_kp(gts),
             "gt_area": np.array([a["area"] for a in gts], dtype=np.float64),
             "gt_bbox": np.ascontiguousarray(np.array([a["bbox"] for a in gts], dtype=np.float64).reshape(-1, 4)),
             "gt_iscrowd": crowd, "gt_ignore": (crowd | nokp).astype(np.int32)}, index, cat)


def coco_pack_gt(gt):
    """The ground-truth half of ``coco_pack``: ``n_images``, ``image_ids`` (ascending) and the ``gt_*`` arrays, the same
    values under the same keys.  This is what ``Engine.coco_open`` uploads once per data set."""
    return _coco_gt(gt)[0]


def coco_stats(precision, recall):
    """COCOeval._summarizeKps on accumulate()'s arrays (precision (10, 101, 3), recall (10, 3); ranges all, medium, large): AP,
    AP50, AP75, AP medium, AP large, then the same five of AR.  Each is the mean over the entries > -1, or -1 without any."""
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    out = []
    for s in (precision, recall):
        out += [mean(s[..., 0]), mean(s[0, ..., 0]), mean(s[5, ..., 0]), mean(s[..., 1]), mean(s[..., 2])]
    return np.array(out, dtype=np.float64)


_default = {}


def default_engine(device_id=None):
    """Shared engine for the free functions (extract_keypoints / group_keypoints / up-sampling)."""
    if device_id is None:
        device_id = 0
    if device_id not in _default:
        _default[device_id] = Engine(device_id)
    return _default[device_id]
