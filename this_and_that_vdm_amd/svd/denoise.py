"""The fused denoise loop: the body of StableVideoDiffusion(ControlNet)Pipeline.__call__'s step loop
(svd/pipeline_stable_video_diffusion_controlnet.py:624-720, VL twin svd/pipeline_stable_video_diffusion.py:528-562)
as ONE hipGraph replayed per step.

Per step, on device:   prep (CFG duplicate, x/sqrt(sigma^2+1), channel concat, NCHW->tokens)  ->  time/FiLM rows
  ->  UNet encoder+mid  ->  GestureNet encoder+mid, zero-convs with the UNet skips added in the epilogue
  ->  UNet decoder  ->  per-frame CFG + v-prediction Euler update of the fp32 latents (in place), or with begin(multistep=...) the
  DPM-Solver++ 2M update (same schedule, one more latent-sized buffer: the previous step's data prediction).
Hoisted out of the loop (step-invariant; the reference recomputes them every step):
context K/V of all 46 cross-attention layers, frame-position embeddings, and the gesture-map latents (the
pipeline VAE-encodes them once instead of 25 times, reference :652).  The time embedding + FiLM rows of all ResBlocks depend
on the schedule only: begin() evaluates them for all steps at once (DenoiserBase.film_table, round 4) and step i copies its
row block into the static buffer the captured epilogues read (TT_FILM_TABLE=0: per step inside the graph, as before).
Step-dependent scalars (sigma_i, sigma_{i+1}, t_i) live in a 3-float device buffer that is refreshed by one
tiny copy before each replay, so a single captured graph serves all steps.  No host sync inside the loop.
Control-guidance windows (reference :611-617,639-645): a step whose ``controlnet_keep`` is 0 multiplies every residual
by 0, i.e. it is exactly the UNet-only step -- such steps replay a second graph that does not launch GestureNet at all."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

import os

from .. import ops
from .layers import Geom

FILM_TABLE = os.environ.get("TT_FILM_TABLE", "1") != "0"

# Most batch elements (requests x CFG batch) one loop can carry.  The time / FiLM rows of a step are one tt_small_linear launch of one row
# per batch element, and that kernel takes at most 32 rows; nothing else in the step is bounded by the batch before this is (the GEMM,
# GroupNorm and attention launches index rows in 64 bits or refuse sizes beyond 2 GiB themselves).  32 allows 16 requests with CFG 2.
MAX_BATCH = 32


class DenoiseLoop:
    def __init__(self, unet, controlnet=None, use_graph: bool = True, split_cfg: bool = False):
        self.unet, self.controlnet, self.use_graph = unet, controlnet, use_graph
        # run the uncond / cond halves as separate concurrent branches too (measured SLOWER on MI355X at 256x448:
        # 47.7 vs 44.4 ms/step -- half-size GEMMs lose more than the overlap wins; kept as an option and tested)
        self.split_cfg = split_cfg
        self.overlap_branches = True        # False: same launches, one stream (used when timing kernels one by one)
        self._streams = {}
        self._graph = None
        self._graph_off = None              # the UNet-only step for controlnet_keep[i] == 0
        self._key = None
        self._static = {}
        self._audit = None                  # the range audit the graphs were captured under (kept alive with them), or None

    # ---- request set-up (everything step-invariant)
    def begin(self, latents: torch.Tensor, image_latents: torch.Tensor, encoder_hidden_states: torch.Tensor,
              added_time_ids: torch.Tensor, guidance_scale: Optional[torch.Tensor], sigmas: torch.Tensor,
              timesteps: torch.Tensor, controlnet_cond: Optional[torch.Tensor] = None, conditioning_scale: float = 1.0,
              controlnet_keep: Optional[Sequence[float]] = None, image_guidance_scale: Optional[float] = None,
              guess_mode: bool = False, multistep: Optional[torch.Tensor] = None):
        """latents [R,F,4,h,w] (already scaled by init_noise_sigma), R independent requests; image_latents [B,F,4,h,w], B = R*C;
        encoder_hidden_states [B,S,D]; added_time_ids [B,3]; guidance_scale [R,F,1,1,1] or [1,F,1,1,1] (all requests), None = no
        CFG (C == 1); sigmas [steps+1], timesteps [steps] (shared by the requests); controlnet_cond gesture latents [F,4,h,w] (all
        requests; the same for every CFG class, reference :660) or [R,F,4,h,w]; controlnet_keep: one 0.0/1.0 per step
        (reference :611-617), None = keep everywhere.  C == 3 is the use_instructpix2pix batch (first-frame, cond, uncond; reference
        :182-184,208-210,698-702) and needs image_guidance_scale.  The batched tensors are in the reference's order, the one
        torch.cat([neg, cond]) gives a batch: CFG class by CFG class, element c * R + r -- which is the loop's internal order too.
        Every request is computed as a begin() of its own would (never the reference's cross-request context pairing).
        guess_mode: the 13 residual scales become
        logspace(-1, 0, 13) * conditioning_scale (temporal_controlnet.py:626-630); only without CFG -- the reference's
        guess-mode + CFG branch (:676-681) concatenates zeros onto an already CFG-sized residual batch and cannot run.
        multistep: None = the Euler update; a [steps] fp32 tensor (DPMSolverMultistepScheduler.multistep_coefficients) = the
        DPM-Solver++ 2M update, every step ending in tt_cfg_multistep_step_requests with that step's coefficient (include/ttvdm.h).
        The previous step's data prediction lives in a static buffer ``x0_hist`` that is never cleared between requests: a step whose
        coefficient is 0 -- the first of every request -- does not read it.  Latents replaced between steps (a pipeline's
        callback_on_step_end) leave the history as it is, as diffusers' multistep schedulers do: the next step extrapolates from the
        data prediction of the latents the loop itself produced."""
        dev = self.unet.device
        b = image_latents.shape[0]
        nr, f, _, h, w = latents.shape
        if b > MAX_BATCH:
            raise ValueError(f"{b} batch elements (requests x CFG batch) in one call; the cap is {MAX_BATCH} "
                             "(the step's time / FiLM rows are one tt_small_linear launch of at most 32 rows)")
        if nr < 1 or b % nr or b // nr not in (1, 2, 3):
            raise ValueError(f"CFG batch must be 1 (no CFG), 2 (uncond, cond) or 3 (use_instructpix2pix): got {b} image-latent "
                             f"batch elements for {nr} request(s)")
        c = b // nr
        if encoder_hidden_states.shape[0] != b or added_time_ids.shape[0] != b:
            raise ValueError(f"encoder_hidden_states ({encoder_hidden_states.shape[0]}) and added_time_ids ({added_time_ids.shape[0]}) "
                             f"need one row block per batch element ({b} = {nr} request(s) x CFG batch {c})")
        if c == 3 and (image_guidance_scale is None or guidance_scale is None):
            raise ValueError("a CFG batch of 3 (use_instructpix2pix) needs guidance_scale and image_guidance_scale")
        if guidance_scale is not None and guidance_scale.numel() not in (f, nr * f):
            raise ValueError(f"guidance_scale holds {guidance_scale.numel()} values: expected [1,F,1,1,1] or [R,F,1,1,1] with "
                             f"R = {nr}, F = {f}")
        if controlnet_cond is not None and controlnet_cond.numel() not in (f * 4 * h * w, nr * f * 4 * h * w):
            raise ValueError(f"controlnet_cond {tuple(controlnet_cond.shape)}: expected [F,4,h,w] or [R,F,4,h,w] with R = {nr}, "
                             f"F = {f}, h = {h}, w = {w}")
        if nr > 1 and self.split_cfg:
            raise NotImplementedError("split_cfg with several requests per call (the option was measured slower; use split_cfg=False)")
        self.unet.prepare()
        self.image_guidance_scale = float(image_guidance_scale) if c == 3 else None
        dtype = self.unet._run_dtype()
        if self.controlnet is not None:
            self.controlnet.prepare()
        # a captured graph holds raw pointers into the models' packed weights: the pack generation of both models is part
        # of the key, so load_state_dict / .to() / in-place updates between requests drop the stale graphs
        packs = self._pack_state()
        key = (nr, b, f, h, w, dtype, self.controlnet is not None, tuple(encoder_hidden_states.shape), len(timesteps),
               guidance_scale is not None, self.image_guidance_scale, packs,   # the image scale is baked into the graph
               ops.f32_split(),                                                # ... and so is the TT_F32 product mode (kernel variants)
               None if ops.AUDIT is None else ops.AUDIT.generation)           # ... and the range audit whose statistics launches a captured step holds
        if multistep is not None:
            if multistep.numel() != len(timesteps):
                raise ValueError(f"multistep holds {multistep.numel()} coefficients for {len(timesteps)} steps: expected one per step")
            if float(multistep.reshape(-1)[0]) != 0.0:
                raise ValueError("multistep[0] must be 0: the first step of a request has no history to extrapolate from")
            key += ("multistep",)               # which step kernel a graph ends in; the coefficient values are data, not structure
        if key != self._key:                    # new shapes or new weights: new static buffers, new graph
            self._graph, self._graph_off, self._key, self._static = None, None, key, {}
        self._packs = packs                     # what the FiLM table, the context projections and the graphs below were built from
        # a graph captured under an audit writes into that audit's records: the loop holds the audit (and so its buffer) for as long as it
        # holds such a graph -- the rule of ops._WS_RETIRED -- and step() refuses to run under another audit, or none, than begin() saw
        self._audit = ops.AUDIT
        self.geom, self.dtype = Geom(b, f, h, w, requests=nr), dtype
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        sig = f32(sigmas)
        # static buffers: a captured graph keeps raw pointers, so later requests are COPIED into the same storage
        self.latents = self._static_set("latents", f32(latents).reshape(f, 4, h, w) if nr == 1 else f32(latents))
        self.image_latents = self._static_set("image_latents", f32(image_latents))
        self.added_time_ids = self._static_set("added_time_ids", f32(added_time_ids))
        self.guidance = self._static_set("guidance", f32(guidance_scale).reshape(-1)) if guidance_scale is not None else None
        self.table = self._static_set("table", torch.stack([sig[:-1], sig[1:], f32(timesteps)], 1))       # [steps, 3]
        self.cur = self._static_set("cur", torch.zeros(3, dtype=torch.float32, device=dev))           # sigma, sigma_next, t
        self.num_steps = self.table.shape[0]
        self.x0_hist = self.coef_tab = self.coef_cur = None
        if multistep is not None:
            # the previous step's data prediction: allocated once per key and left as it is between requests (step 0's coefficient is 0)
            self.x0_hist = self._static.get("x0_hist")
            if self.x0_hist is None:
                self.x0_hist = self._static["x0_hist"] = torch.zeros_like(self.latents)
            self.coef_tab = self._static_set("coef_tab", f32(multistep).reshape(-1))                      # [steps]
            self.coef_cur = self._static_set("coef_cur", torch.zeros(1, dtype=torch.float32, device=dev))   # this step's (copied in by step())
        self.film_tab_u = self.film_tab_c = self.film_cur_u = self.film_cur_c = None
        if FILM_TABLE:
            self.film_tab_u = self._static_set("film_tab_u", self.unet.film_table(self.table[:, 2], self.added_time_ids, b))
            self.film_cur_u = self._static_set("film_cur_u", self.film_tab_u[0])
        ehs = encoder_hidden_states.to(dev)
        k, vt, s, sp, zmask = self.unet.project_context(ehs)
        if self._static.setdefault("zero_ctx_mask", zmask) != zmask:
            self._graph = self._graph_off = None        # which rows skip cross-attention is part of the launch structure
            self._static["zero_ctx_mask"] = zmask
        self.ctx_unet = (self._static_set("k_unet", k), self._static_set("vt_unet", vt), s, sp, zmask)
        self.req_unet = self._request_major("unet", self.ctx_unet, nr, c)
        self.cond = self.req_cn = None
        if self.controlnet is not None:
            if guess_mode and c > 1:
                raise NotImplementedError("guess_mode with CFG (the reference's branch :676-681 cannot run either)")
            if controlnet_cond is None:
                raise ValueError("controlnet_cond (VAE-encoded gesture latents) is required with a ControlNet")
            self.controlnet.prepare()
            if self.controlnet._run_dtype() != self.dtype:
                raise RuntimeError("UNet and ControlNet must run in the same 16-bit dtype inside the fused loop")
            self.cond = self._static_set("cond", f32(controlnet_cond).reshape(-1, 4, h, w))
            if FILM_TABLE:
                self.film_tab_c = self._static_set("film_tab_c", self.controlnet.film_table(self.table[:, 2], self.added_time_ids, b))
                self.film_cur_c = self._static_set("film_cur_c", self.film_tab_c[0])
            k, vt, s, sp, zmask_cn = self.controlnet.project_context(ehs)
            if self._static.setdefault("zero_ctx_mask_cn", zmask_cn) != zmask_cn:
                self._graph = self._graph_off = None
                self._static["zero_ctx_mask_cn"] = zmask_cn
            self.ctx_cn = (self._static_set("k_cn", k), self._static_set("vt_cn", vt), s, sp, zmask_cn)
            self.req_cn = self._request_major("cn", self.ctx_cn, nr, c)
            self.cn_scales = self.controlnet._scales(float(conditioning_scale), bool(guess_mode), len(self.controlnet.controlnet_down_blocks))
            if self._static.setdefault("cn_scales", self.cn_scales) != self.cn_scales:
                self._graph = None              # the scale is a launch argument baked into the graph
                self._static["cn_scales"] = self.cn_scales
        self.keep = [1.0] * self.num_steps if controlnet_keep is None else [float(v) for v in controlnet_keep]
        if len(self.keep) != self.num_steps or any(v not in (0.0, 1.0) for v in self.keep):
            raise ValueError("controlnet_keep needs one 0.0/1.0 entry per step")
        self.step_index = 0
        return self

    def _pack_state(self, repack: bool = True):
        """(identity, pack generation, fp8 switch) of both models: prepare() bumps the generation on every repack.
        repack=True (begin): prepare() first, so parameters that changed since the last pack are re-packed now.
        repack=False (step): nothing is packed; a model whose parameters no longer match its pack (in-place update, .to(),
        load_state_dict, invalidate_packs) reports generation -1, which never equals what begin() recorded."""
        st = ()
        for m in (self.unet, self.controlnet):
            if m is None:
                continue
            if repack:
                m.prepare()
            fresh = repack or getattr(m, "_packed_key", None) == m._pack_key()
            st += (id(m), m._pack_gen if fresh else -1, bool(m.attention_fp8))
        return st

    def _request_major(self, name: str, ctx, nr: int, c: int):
        """(K, V^T) with the contexts re-ordered request by request (r * C + c) for the temporal cross-attention's per-request
        launches; None where the loop's own order serves (one request, or no CFG)."""
        if nr == 1 or c == 1:
            return None
        k, vt, _, sp, _ = ctx
        k_req = k.view(c, nr, sp, -1).transpose(0, 1).reshape(k.shape)
        vt_req = vt.view(-1, c, nr, sp).transpose(1, 2).reshape(vt.shape)
        return (self._static_set("k_req_" + name, k_req), self._static_set("vt_req_" + name, vt_req))

    def _static_set(self, name: str, value: torch.Tensor) -> torch.Tensor:
        cur = self._static.get(name)
        if cur is not None and cur.shape == value.shape and cur.dtype == value.dtype:
            cur.copy_(value)
            return cur
        self._static[name] = value.clone()          # never alias the caller's tensor: latents are updated in place
        if cur is not None:
            self._graph = self._graph_off = None
        return self._static[name]

    # ---- one step's launches (captured once)
    def _launch_step(self, use_cn: bool = True):
        if ops.AUDIT is None:
            return self._launch_step_branches(use_cn)
        # under a range audit every step names its sites alike: the ordinals restart where the first step started them
        with ops.AUDIT.region("step" if use_cn or self.controlnet is None else "step.unet_only"):
            return self._launch_step_branches(use_cn)

    def _launch_step_branches(self, use_cn: bool = True):
        """One step as concurrent branches (fork/join with events; captured as parallel hipGraph branches).
        GestureNet's encoder+mid is independent of the UNet's until the zero-convs, so the two run side by side: the
        latency-bound small kernels and the tails of one branch fill the idle CUs of the other (49.8 -> 44.4 ms/step).
        With ``split_cfg`` the uncond / cond halves (which never interact inside the networks) become branches too."""
        g = self.geom
        cn = self.controlnet if use_cn else None
        from . import layers as _layers
        _layers._Side.origin = torch.cuda.current_stream().cuda_stream     # the only stream that may fork side launches under capture
        cpad = cn._cin_pad if cn is not None else self.unet._cin_pad
        if g.requests == 1:
            x_tok = ops.prep_model_input(self.latents, self.image_latents, self.cond if use_cn else None, self.cur, 0, g.batch, g.frames, g.h, g.w,
                                         cpad, self.dtype)
        else:
            x_tok = ops.prep_model_input_requests(self.latents, self.image_latents, self.cond if use_cn else None, self.cur, 0, g.requests,
                                                  g.cfg, g.frames, g.h, g.w, cpad, self.dtype)
        t = self.cur[2:3]
        x_unet = x_tok if cpad == self.unet._cin_pad else x_tok[:, :self.unet._cin_pad]
        if self.film_cur_u is not None:         # this step's rows of the per-request FiLM table (copied in by step())
            ctx_u = self.unet._step_context(None, self.ctx_unet, film=self.film_cur_u, request_ctx=self.req_unet)
        else:
            ctx_u = self.unet._step_context(self.unet._embed(t, self.added_time_ids, g.batch, x_tok.device), self.ctx_unet,
                                            request_ctx=self.req_unet)
        ctx_c = None
        if cn is not None:
            if self.film_cur_c is not None:
                ctx_c = cn._step_context(None, self.ctx_cn, film=self.film_cur_c, request_ctx=self.req_cn)
            else:
                ctx_c = cn._step_context(cn._embed(t, self.added_time_ids, g.batch, x_tok.device), self.ctx_cn, request_ctx=self.req_cn)
        eps = torch.empty((g.m, self.unet.conv_out.out_channels), dtype=torch.float32, device=x_tok.device)
        halves = [Geom(1, g.frames, g.h, g.w, b, g.batch) for b in range(g.batch)] if self.split_cfg and g.batch > 1 else [g]
        rows = halves[0].m
        main = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(main)
        tails = []
        for i, gh in enumerate(halves):
            su = main if i == 0 else self._stream(f"u{i}")
            lo, hi_ = i * rows, (i + 1) * rows
            join = None
            if cn is not None:
                sc = self._stream(f"c{i}")
                sc.wait_event(fork)
                with torch.cuda.stream(sc):
                    cn_skips, cn_mid, _ = cn.encode_tokens(x_tok[lo:hi_], gh, ctx_c)
                    join = torch.cuda.Event()
                    join.record(sc)
            if su is not main:
                su.wait_event(fork)
            with torch.cuda.stream(su):
                x, gm, skips = self.unet.encode_tokens(x_unet[lo:hi_], gh, ctx_u)
                if cn is not None:
                    su.wait_event(join)
                    skips, (x, _) = cn.zero_convs(cn_skips, cn_mid, gm, self.cn_scales, add_to=([s for s, _ in skips], x))
                self.unet.decode_tokens(x, gm, skips, ctx_u, eps_out=eps[lo:hi_])
                if su is not main:
                    done = torch.cuda.Event()
                    done.record(su)
                    tails.append(done)
        for ev in tails:
            main.wait_event(ev)
        if self.x0_hist is not None:            # DPM-Solver++ 2M: one kernel for every R (the request form serves R = 1 too)
            ops.cfg_multistep_step_requests(eps, self.latents, self.x0_hist, self.guidance, self.cur, 0, self.coef_cur, g.requests, g.cfg,
                                            g.frames, g.h, g.w, self.image_guidance_scale)
        elif g.requests == 1:
            ops.cfg_euler_step(eps, self.latents, self.guidance, self.cur, 0, g.batch, g.frames, g.h, g.w,
                               self.image_guidance_scale)
        else:
            ops.cfg_euler_step_requests(eps, self.latents, self.guidance, self.cur, 0, g.requests, g.cfg, g.frames, g.h, g.w,
                                        self.image_guidance_scale)

    def _stream(self, name):
        if not self.overlap_branches:
            return torch.cuda.current_stream()
        st = self._streams.get(name)
        if st is None:
            st = self._streams[name] = torch.cuda.Stream()
        return st

    def step(self):
        """Advance the latents by one step, Euler or (begin(multistep=...)) DPM-Solver++ 2M (asynchronous; call torch.cuda.synchronize() to wait)."""
        if self.step_index >= self.num_steps:
            raise RuntimeError("denoise loop already finished; call begin() for a new request")
        # begin() evaluated the FiLM rows of ALL steps and the context K/V from the weights of that moment, and the captured graph
        # holds pointers into that pack: a weight reload / repack between begin() and step() must not be served from them
        if self._pack_state(repack=False) != self._packs:
            raise RuntimeError("model weights were re-packed (load_state_dict / .to() / in-place update) after DenoiseLoop.begin(): "
                               "call begin() again -- the per-request FiLM table and context projections belong to the old weights")
        if ops.AUDIT is not self._audit:
            raise RuntimeError("a range audit began or ended after DenoiseLoop.begin(): call begin() again -- a captured step holds the "
                               "statistics launches of the audit it was captured under, or none")
        self.cur.copy_(self.table[self.step_index])
        if self.coef_cur is not None:
            self.coef_cur.copy_(self.coef_tab[self.step_index:self.step_index + 1])
        use_cn = self.controlnet is not None and self.keep[self.step_index] != 0.0
        if self.film_cur_u is not None:
            self.film_cur_u.copy_(self.film_tab_u[self.step_index])
            if use_cn:
                self.film_cur_c.copy_(self.film_tab_c[self.step_index])
        if not self.use_graph:
            self._launch_step(use_cn)
        elif use_cn or self.controlnet is None:
            if self._graph is None:
                self._graph = self._capture(self.controlnet is not None)
            self._graph.replay()
        else:
            if self._graph_off is None:
                self._graph_off = self._capture(False)
            self._graph_off.replay()
        self.step_index += 1

    def _capture(self, use_cn: bool):
        # warm-up on a side stream (allocator + lazily built caches), restoring the latents afterwards -- and the multistep history: the
        # UNet-only graph of a control-guidance window is first captured in the middle of a request, where the replay that follows reads
        # the data prediction of the step before, not the warm-up's
        keep = self.latents.clone()
        keep_hist = None if self.x0_hist is None else self.x0_hist.clone()
        records = None if ops.AUDIT is None else ops.AUDIT.snapshot()         # the warm-up pass below is not a step of the request: its
        s = torch.cuda.Stream()                                                # statistics are taken back out of the audit's records
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._launch_step(use_cn)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._launch_step(use_cn)
        self.latents.copy_(keep)
        if keep_hist is not None:
            self.x0_hist.copy_(keep_hist)
        if ops.AUDIT is not None:
            ops.AUDIT.restore(records)
        return graph

    def run(self, steps: Optional[int] = None) -> torch.Tensor:
        n = self.num_steps - self.step_index if steps is None else steps
        for _ in range(n):
            self.step()
        return self.result()

    def result(self) -> torch.Tensor:
        g = self.geom
        return self.latents.view(g.requests, g.frames, 4, g.h, g.w)
