"""CPU stand-in for a beam session that offers wlk_decode_beam_until_stop, for TESTS ONLY: the LIBRARY's own host logic
of the beam loop (wlk_beam_job_*: budget, adjustments, BeamSearchDecoder.update, stop rules) driven with the oracle's
numerics in place of the kernels - what fake_session.FakeSession.decode_until_stop is for beam 1."""
import ctypes as C

import numpy as np

from fake_session import FakeHipModel, FakeSession


class BeamLoopFakeSession(FakeSession):
    def decode_beam_until_stop(self, tokens, params, suppress_ids, blank_ids):
        from whisperlivekit_amd import _lib
        from whisperlivekit_amd.engine import LoopOutcome
        lib = _lib.load()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        B, K = self.beam, self.beam + 1
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        sup = np.ascontiguousarray(suppress_ids, dtype=np.int32)
        blank = np.ascontiguousarray(blank_ids, dtype=np.int32)
        job = C.c_void_p()
        _lib.check(lib.wlk_beam_job_create(C.byref(params), B, vp(t), t.size, vp(sup), sup.size, vp(blank), blank.size,
                                           C.byref(job)))
        rows = np.tile(t, (B, 1))
        first = True
        try:
            while True:
                n_feed = C.c_int32()
                _lib.check(lib.wlk_beam_job_begin_step(job, C.byref(n_feed)))
                if n_feed.value == 0:
                    break
                assert n_feed.value == (rows.shape[1] if first else 1)
                self.decode(rows if first else rows[:, -1:], first=first, sot_index=int(params.sot_index))
                if first and params.no_speech_token >= 0:
                    stops = C.c_int32()
                    prob = float(self.no_speech_prob(int(params.no_speech_token))[0])
                    _lib.check(lib.wlk_beam_job_no_speech(job, prob, C.byref(stops)))
                    if stops.value:
                        break
                first = False
                ids_p, dl_p, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int32()
                _lib.check(lib.wlk_beam_job_adjustments(job, C.byref(ids_p), C.byref(dl_p), C.byref(n)))
                ids = [ids_p[i] for i in range(n.value)]
                dls = [dl_p[i] for i in range(n.value)]
                assert len(set(ids)) == len(ids)
                lp, top, frames = self.select([-1] * len(ids), ids, dls, K, int(params.content_mel_len))
                lp = np.ascontiguousarray(lp, np.float32)
                top = np.ascontiguousarray(top, np.int32)
                frames = np.ascontiguousarray(frames, np.int32)
                go = C.c_int32()
                _lib.check(lib.wlk_beam_job_consume(job, vp(lp), vp(top), vp(frames), C.byref(go)))
                n_len = C.c_int32()
                rows = np.empty((B, rows.shape[1] + 1), np.int64)
                src = np.empty(B, np.int32)
                _lib.check(lib.wlk_beam_job_state(job, vp(rows), rows.size, C.byref(n_len), None, vp(src), None))
                assert n_len.value == rows.shape[1]
                if not go.value:
                    break
                if src.tolist() != list(range(B)):
                    self.kv_reorder(src.tolist())
            cap = int(params.max_text_len) + 8
            res = _lib.LoopResult()
            new = np.empty(cap, np.int64)
            st, sf, ss = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float32)
            _lib.check(lib.wlk_beam_job_result(job, C.byref(res), vp(new), vp(st), vp(sf), vp(ss), cap))
            return LoopOutcome(res, new, st, sf, ss)
        finally:
            lib.wlk_beam_job_destroy(job)


class BeamLoopFakeModel(FakeHipModel):
    def new_session(self, beam=1, max_audio_seconds=64.0):
        return BeamLoopFakeSession(self, beam)
