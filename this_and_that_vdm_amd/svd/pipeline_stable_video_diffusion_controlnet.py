"""StableVideoDiffusionControlNetPipeline (VGL) -- drop-in for
svd/pipeline_stable_video_diffusion_controlnet.py:371-736 with the 25-step loop executed by the fused,
hipGraph-replayed DenoiseLoop (svd/denoise.py).

Kept: the ``__call__`` surface and argument meaning, CLIP(+text) context with the freshly constructed
LayerNorm((78,1024)) (reference :165-173), un-scaled VAE ``.mode()`` latents (:200), CFG order [uncond, cond]
(:177-185,203-211), fps-1 / motion bucket / noise-aug time ids, per-frame guidance ramp, ``output_type="latent"``,
``latents=``, ``generator=``, ``callback_on_step_end``, a list of images and ``num_videos_per_prompt`` (one call carries
R = images x videos-per-image independent requests, image-major; every video is what a call of its own would give -- DESIGN.md section 8).
Opt-in (``native_image_io=True``, default off): the CLIP image preprocessing, the use_text context LayerNorm and the export of decoded
frames run on the library's kernels (ops.clip_image / layernorm_block / frames_out) instead of stock torch ops; RGB PIL / uint8 images
are uploaded once, as uint8, and the VAE input (PIL's LANCZOS resize, 2 x - 1, the noise augmentation) is ops.vae_image on that upload;
``image=DevicePixels(...)`` takes pixels that are on the device already, and ``output_type="device"`` returns the uint8 frames
[R, F, H, W, C] as a device tensor (what "pil" holds, never copied to the host: export.write_gif / metrics.compare_frames take it).
``use_instructpix2pix`` (CFG batch of 3, reference :182-184,208-210,698-702) and ``guess_mode`` without CFG are built;
``guess_mode`` with CFG raises, as the reference's branch (:676-681) cannot run either.
Changed on purpose: the gesture map is VAE-encoded ONCE per request instead of inside every step (reference :652 --
loop-invariant), in the VAE's own dtype after the force_upcast window, exactly where the reference encodes it."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Union

import numpy as np
import PIL.Image
import torch
import torch.nn as nn

from .. import ops
from ..gesture_map import GesturePoints, rasterise_points_device
from .denoise import DenoiseLoop
from .pipeline_utils import (CLIPFeatureExtractor, DevicePixels, PipelineBase, StableVideoDiffusionPipelineOutput, VaeImageProcessor,
                             append_dims, randn_tensor, resize_with_antialiasing, tensor2vid)
from .temporal_controlnet import ControlNetModel


_NO_FEATURE_EXTRACTOR = ("encode_clip: the pipeline has no feature_extractor, so the CLIP mean/std normalisation the "
                         "reference always applies (:145-152) cannot be done; build the pipeline with from_pretrained() "
                         "or pass feature_extractor=CLIPFeatureExtractor()")


class _SVDPipelineCore(PipelineBase):
    model_cpu_offload_seq = "image_encoder->unet->vae"
    _callback_tensor_inputs = ["latents"]
    native_image_io = False            # class default: also what an instance built without __init__ sees
    range_audit = False                # True: every call runs under an audit.RangeAudit and leaves its report in last_range_audit
    last_range_audit = None

    def __init__(self, vae, image_encoder, unet, scheduler, feature_extractor, native_image_io: bool = False, range_audit: bool = False):
        self.register_modules(vae=vae, image_encoder=image_encoder, unet=unet, scheduler=scheduler,
                              feature_extractor=feature_extractor)
        # True: PIL / numpy images reach CLIP through ops.clip_image, the use_text context LayerNorm is ops.layernorm_block and
        # "np" / "pil" frames leave through ops.frames_out (one uint8 / fp32 NHWC copy per decoded chunk).  A plain attribute:
        # it may be switched between calls.
        self.native_image_io = bool(native_image_io)
        # True: a call runs CLIP encode, VAE encode, the denoise loop and the decode under ONE range audit (audit.py) -- every tensor the
        # kernels write is followed by a statistics pass, frames and latents stay bit-equal -- and the report (sites of image_encoder.*,
        # text_encoder.*, vae.*, unet.*, controlnet.*) is left in ``last_range_audit``.  A diagnostic mode; a plain attribute as well.
        self.range_audit = bool(range_audit)
        self.last_range_audit = None
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_convert_rgb=True)
        self.control_image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_convert_rgb=True,
                                                         do_normalize=False)
        self._loops: Dict[bool, DenoiseLoop] = {}

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, *, vae=None, image_encoder=None, unet=None, scheduler=None,
                        feature_extractor=None, torch_dtype=None, native_image_io: bool = False, range_audit: bool = False, **kwargs):
        """The reference passes vae / image_encoder / unet explicitly (test_code/inference.py:171-178) and lets diffusers
        load the remaining components from the hub folder.  Same here, from a LOCAL diffusers-format folder (no network):
          feature_extractor/preprocessor_config.json -> CLIP image processor (mean/std used by ``encode_clip``, reference :145-152)
          scheduler/scheduler_config.json            -> EulerDiscreteScheduler
          unet/                                      -> UNetSpatioTemporalConditionModel (only if ``unet`` is not passed)
        vae and image_encoder are third-party models (AutoencoderKLTemporalDecoder / CLIPVisionModelWithProjection) and must be
        passed in.  Without a folder the scheduler defaults to SVD's shipped EulerDiscrete configuration and the feature
        extractor to CLIP's published preprocessing constants; nothing is ever silently skipped.
        ``native_image_io=True`` sets the pipeline attribute of that name (default False: the torch request path), ``range_audit=True``
        the attribute of that name (default False: no statistics launches)."""
        import os
        path = pretrained_model_name_or_path
        have_dir = isinstance(path, str) and os.path.isdir(path)
        if unet is None and have_dir and os.path.isdir(os.path.join(path, "unet")):
            from .unet_spatio_temporal_condition import UNetSpatioTemporalConditionModel
            unet = UNetSpatioTemporalConditionModel.from_pretrained(path, subfolder="unet", torch_dtype=torch_dtype)
        missing = [n for n, v in (("vae", vae), ("image_encoder", image_encoder), ("unet", unet)) if v is None]
        if missing:
            raise ValueError(f"{cls.__name__}.from_pretrained needs these components passed in: {missing}")
        if scheduler is None:
            from .scheduling_euler_discrete import EulerDiscreteScheduler
            cfg = os.path.join(path, "scheduler", "scheduler_config.json") if have_dir else None
            scheduler = EulerDiscreteScheduler.from_config(cfg) if cfg and os.path.isfile(cfg) else EulerDiscreteScheduler()
        if feature_extractor is None:
            cfg = os.path.join(path, "feature_extractor", "preprocessor_config.json") if have_dir else None
            feature_extractor = CLIPFeatureExtractor.from_json_file(cfg) if cfg and os.path.isfile(cfg) else CLIPFeatureExtractor()
        return cls(vae=vae, image_encoder=image_encoder, unet=unet, scheduler=scheduler, feature_extractor=feature_extractor,
                   native_image_io=native_image_io, range_audit=range_audit)

    # ---- constants of a request (reference :130-254,305-337)
    def encode_clip(self, image, prompt, use_text, text_encoder, device, num_videos_per_prompt, do_classifier_free_guidance,
                    use_instructpix2pix=False):
        dtype = next(self.image_encoder.parameters()).dtype
        # encode_clip needs only the encoder, the two processors and, optionally, this switch of whatever object it is called on
        # (callers run it unbound on stand-ins that predate the option): absent means off
        native = getattr(self, "native_image_io", False)
        if not isinstance(image, torch.Tensor):
            if native:
                image = self._clip_image_native(image, device, dtype)
            else:
                image = self.image_processor.numpy_to_pt(self.image_processor.pil_to_numpy(image))
                image = (resize_with_antialiasing(image * 2.0 - 1.0, (224, 224)) + 1.0) / 2.0
                if self.feature_extractor is None:
                    raise RuntimeError(_NO_FEATURE_EXTRACTOR)
                image = self.feature_extractor(images=image, do_normalize=True, do_center_crop=False, do_resize=False,
                                               do_rescale=False, return_tensors="pt").pixel_values
        emb = self.image_encoder(image.to(device=device, dtype=dtype)).image_embeds.unsqueeze(1)
        bs, seq, _ = emb.shape
        ehs = emb.repeat(1, num_videos_per_prompt, 1).view(bs * num_videos_per_prompt, seq, -1)
        if use_text:
            text = text_encoder(prompt)[0]
            if bs * num_videos_per_prompt != 1:
                # one row of ids per image (repeated for its videos, like the image embedding above), or one row for all requests
                if text.shape[0] == bs:
                    text = text.repeat_interleave(num_videos_per_prompt, 0)
                elif text.shape[0] == 1:
                    text = text.expand(bs * num_videos_per_prompt, -1, -1)
                else:
                    raise ValueError(f"prompt: {text.shape[0]} rows of token ids for {bs} image(s); pass one row per image or one row "
                                     "for all")
            ehs = torch.cat((text, ehs), dim=1)
            if native:
                ehs = ops.layernorm_block(ehs.reshape(-1, ehs.shape[-1]), ehs.shape[1], eps=1e-5).view(ehs.shape)
            else:
                ln = nn.LayerNorm(tuple(ehs.shape[1:])).to(device=device, dtype=dtype)      # fresh, gamma=1 beta=0 (:172)
                ehs = ln(ehs)
        if do_classifier_free_guidance:
            neg = torch.zeros_like(ehs)
            ehs = torch.cat([ehs, neg, neg]) if use_instructpix2pix else torch.cat([neg, ehs])        # :182-185
        return ehs

    def _clip_image_native(self, image, device, dtype):
        """PIL / list of PIL / numpy image(s) -> the CLIP vision model's input on the device: the uint8 HWC pixels are uploaded once
        and ops.clip_image does the reference's resize + normalisation (:145-152, 741-767) there.  A numpy image that is not uint8
        takes the values pil_to_numpy would give it (x / 255), as float32 NCHW.  The images must be RGB (three channels): the kernel
        refuses anything else, where the torch path would hand a grayscale / RGBA array on to the encoder."""
        if self.feature_extractor is None:
            raise RuntimeError(_NO_FEATURE_EXTRACTOR)
        if isinstance(image, DevicePixels):                     # the request's one upload (_request_pixels), or the caller's own pixels
            return ops.clip_image(image.pixels, (224, 224), self.feature_extractor.image_mean, self.feature_extractor.image_std, dtype)
        ims = [np.asarray(im) for im in (image if isinstance(image, (list, tuple)) else [image])]
        arr = np.stack([im[..., None] if im.ndim == 2 else im for im in ims], 0)
        if arr.dtype == np.uint8:
            src = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        else:
            src = self.image_processor.numpy_to_pt(arr.astype(np.float32) / 255.0).contiguous().to(device)
        return ops.clip_image(src, (224, 224), self.feature_extractor.image_mean, self.feature_extractor.image_std, dtype)

    def _request_pixels(self, image, device):
        """The uint8 pixels of a request on the device, uploaded ONCE for both of their readers (_clip_image_native and ops.vae_image),
        when ``native_image_io`` is on and the image is what the kernels take: DevicePixels, RGB PIL image(s), or a list of uint8
        [H, W, 3] arrays.  None otherwise (tensors, float arrays, other PIL modes, the option off): today's host path, unchanged."""
        if isinstance(image, DevicePixels):
            if not self.native_image_io:
                raise ValueError("image=DevicePixels needs a pipeline with native_image_io=True: the torch request path starts from host "
                                 "images (PIL / numpy / tensor)")
            return image if image.device == torch.device(device) else DevicePixels(image.pixels.to(device))
        if not self.native_image_io:
            return None
        ims = image if isinstance(image, list) else [image]
        if not ims or not all((isinstance(im, PIL.Image.Image) and im.mode == "RGB" and im.size == ims[0].size)
                              or (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3
                                  and im.shape == ims[0].shape) for im in ims):
            return None
        return DevicePixels.from_pil(ims, device)

    def _encode_vae_image(self, image, device, num_videos_per_prompt, do_classifier_free_guidance, use_instructpix2pix=False):
        lat = self.vae.encode(image.to(device=device)).latent_dist.mode()
        if do_classifier_free_guidance:
            neg = torch.zeros_like(lat)
            lat = torch.cat([lat, lat, neg]) if use_instructpix2pix else torch.cat([neg, lat])        # :208-211
        return lat.repeat(num_videos_per_prompt, 1, 1, 1)

    def _get_add_time_ids(self, fps, motion_bucket_id, noise_aug_strength, dtype, batch_size, num_videos_per_prompt,
                          do_classifier_free_guidance, guess_mode=False, use_instructpix2pix=False):
        ids = [fps, motion_bucket_id, noise_aug_strength]
        passed = self.unet.config.addition_time_embed_dim * len(ids)
        expected = self.unet.add_embedding.linear_1.in_features
        if expected != passed:
            raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of {passed} "
                             "was created. The model has an incorrect config.")
        t = torch.tensor([ids], dtype=dtype).repeat(batch_size * num_videos_per_prompt, 1)
        if not do_classifier_free_guidance:
            return t
        return torch.cat([t, t, t]) if use_instructpix2pix else torch.cat([t, t])

    def _decode_chunks(self, latents, decode_chunk_size):
        """the decoder's ``.sample`` [f, 3, H, W] for every chunk of at most decode_chunk_size frames (reference :257-283), video by
        video: a chunk never spans two videos (the reference chunks flatten(0, 1); the temporal decoder mixes the frames of a
        chunk, so a video of a batched call would otherwise depend on its neighbour)"""
        import inspect
        takes_frames = "num_frames" in inspect.signature(self.vae.forward).parameters
        for video in latents:
            lat = video / self.vae.config.scaling_factor
            for i in range(0, lat.shape[0], decode_chunk_size):
                chunk = lat[i:i + decode_chunk_size]
                kw = {"num_frames": chunk.shape[0]} if takes_frames else {}
                yield self.vae.decode(chunk, **kw).sample

    def decode_latents(self, latents, num_frames, decode_chunk_size=14):
        frames = torch.cat(list(self._decode_chunks(latents, decode_chunk_size)), 0)
        return frames.reshape(-1, num_frames, *frames.shape[1:]).permute(0, 2, 1, 3, 4).float()

    def _frames_native(self, latents, num_frames, decode_chunk_size, output_type):
        """decode_latents + tensor2vid for "np" / "pil" through ops.frames_out: every decoded chunk leaves the device once, as the
        NHWC float32 ("np") or uint8 ("pil") array the caller receives."""
        kind = 0 if output_type == "np" else 1
        host = [ops.frames_out(sample, kind).cpu().numpy() for sample in self._decode_chunks(latents, decode_chunk_size)]
        arr = np.concatenate(host, 0)
        arr = arr.reshape(-1, num_frames, *arr.shape[1:])                                # [B, F, H, W, C]
        if output_type == "np":
            return arr
        return [[PIL.Image.fromarray(im.squeeze(-1) if im.shape[-1] == 1 else im) for im in video] for video in arr]

    def _frames_device(self, latents, num_frames, decode_chunk_size):
        """output_type "device": the uint8 chunks ops.frames_out(sample, 1) writes for "pil", concatenated ON the device -> uint8
        [R, F, H, W, C]; no host copy.  export.write_gif and metrics.compare_frames take it as it is."""
        frames = torch.cat([ops.frames_out(sample, 1) for sample in self._decode_chunks(latents, decode_chunk_size)], 0)
        return frames.reshape(-1, num_frames, *frames.shape[1:])

    def check_inputs(self, image, height, width):
        if not isinstance(image, (torch.Tensor, PIL.Image.Image, list, DevicePixels)):
            raise ValueError("`image` has to be of type `torch.FloatTensor` or `PIL.Image.Image` or `List[PIL.Image.Image]` "
                             f"but is {type(image)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")

    def prepare_latents(self, batch_size, num_frames, num_channels_latents, height, width, dtype, device, generator, latents=None,
                        scheduler=None):
        shape = (batch_size, num_frames, num_channels_latents // 2, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective "
                             f"batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
        latents = randn_tensor(shape, generator=generator, device=device, dtype=dtype) if latents is None else latents.to(device)
        return latents * (self.scheduler if scheduler is None else scheduler).init_noise_sigma

    def prepare_condition_image(self, condition_img, device):
        """[0,1] float gesture frames [F,3,H,W] -> fp16 on device (reference :363-364, quirk Q7).  A list of such arrays, or one
        [N,F,3,H,W] array, holds one gesture map per image."""
        if isinstance(condition_img, (list, tuple)):
            return torch.stack([self.prepare_condition_image(c, device) for c in condition_img], 0)
        t = torch.from_numpy(condition_img) if isinstance(condition_img, np.ndarray) else condition_img
        return t.to(torch.float16).to(device)

    def _encode_gesture_maps(self, cond, num_videos_per_prompt):
        """prepared gesture frames -> VAE latents: [F,3,H,W] -> [F,4,h,w] (shared by every request); one map per image
        [N,F,3,H,W] -> [N * num_videos_per_prompt,F,4,h,w], each image's latents repeated for its videos.  ONE encode per call."""
        lat = self.vae.encode(cond.reshape(-1, *cond.shape[-3:]).to(self.vae.dtype)).latent_dist.mode()
        if cond.ndim == 5:
            lat = lat.reshape(cond.shape[0], cond.shape[1], *lat.shape[1:]).repeat_interleave(num_videos_per_prompt, 0)
        return lat

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def num_timesteps(self):
        return self._num_timesteps

    # ---- the shared generation routine
    def _generate(self, image, condition_img, controlnet, prompt, use_text, text_encoder, *args, **kwargs):
        """``range_audit`` off (the default): the request as it is.  On: the same request under one audit.RangeAudit whose report is left
        in ``last_range_audit`` (also when the request raises: the report then ends where the call did)."""
        if not getattr(self, "range_audit", False):
            return self._generate_request(image, condition_img, controlnet, prompt, use_text, text_encoder, *args, **kwargs)
        from .. import audit
        with audit.RangeAudit() as a:
            for root, model in (("image_encoder", self.image_encoder), ("text_encoder", text_encoder), ("vae", self.vae), ("unet", self.unet),
                                ("controlnet", controlnet)):
                if isinstance(model, torch.nn.Module):
                    a.watch(model, root)
            try:
                return self._generate_request(image, condition_img, controlnet, prompt, use_text, text_encoder, *args, **kwargs)
            finally:
                self.last_range_audit = a.report()

    @torch.no_grad()
    def _generate_request(self, image, condition_img, controlnet, prompt, use_text, text_encoder, height, width, num_frames,
                  num_inference_steps, min_guidance_scale, max_guidance_scale, fps, motion_bucket_id, noise_aug_strength,
                  decode_chunk_size, num_videos_per_prompt, generator, latents, output_type, callback_on_step_end,
                  callback_on_step_end_tensor_inputs, return_dict, controlnet_conditioning_scale=1.0,
                  control_guidance_start=0.0, control_guidance_end=1.0, use_instructpix2pix=False, image_guidance_scale=7.5,
                  guess_mode=False):
        rq = self._request_setup(image, condition_img, controlnet, prompt, use_text, text_encoder, height, width, num_frames,
                                 num_inference_steps, min_guidance_scale, max_guidance_scale, fps, motion_bucket_id, noise_aug_strength,
                                 num_videos_per_prompt, generator, latents, use_instructpix2pix, self.scheduler)
        num_frames, do_cfg, ip2p, ehs, latents, timesteps = rq.num_frames, rq.do_cfg, rq.ip2p, rq.ehs, rq.latents, rq.timesteps
        decode_chunk_size = decode_chunk_size if decode_chunk_size is not None else num_frames
        self._guidance_scale = rq.guidance
        self._num_timesteps = len(timesteps)
        scale = controlnet_conditioning_scale[0] if isinstance(controlnet_conditioning_scale, list) else controlnet_conditioning_scale

        # which steps keep the ControlNet (reference :611-617): 0.0 outside [start, end], else 1.0
        n = len(timesteps)
        keep = [1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end) for i in range(n)]

        key = controlnet is not None
        loop = self._loops.get(key)
        if loop is None or loop.controlnet is not controlnet or loop.unet is not self.unet:
            loop = self._loops[key] = DenoiseLoop(self.unet, controlnet, use_graph=True)
        loop.begin(latents=latents, image_latents=rq.image_latents, encoder_hidden_states=ehs, added_time_ids=rq.added_time_ids,
                   guidance_scale=rq.guidance if do_cfg else None, sigmas=self.scheduler.sigmas, timesteps=timesteps,
                   controlnet_cond=rq.gesture_latents, conditioning_scale=float(scale),
                   controlnet_keep=keep if controlnet is not None else None,
                   image_guidance_scale=float(image_guidance_scale) if ip2p else None,
                   guess_mode=bool(guess_mode) and controlnet is not None, **rq.sampler)
        with self.progress_bar(total=num_inference_steps) as bar:
            for i, t in enumerate(timesteps):
                loop.step()
                if callback_on_step_end is not None:
                    cur = loop.result().to(latents.dtype)
                    outs = callback_on_step_end(self, i, t, {k: cur for k in callback_on_step_end_tensor_inputs if k == "latents"})
                    new = (outs or {}).pop("latents", None)
                    if new is not None and new is not cur:
                        loop.latents.copy_(new.reshape(loop.latents.shape))
                bar.update()
        frames = self._request_finish(loop.result().to(ehs.dtype), num_frames, decode_chunk_size, output_type)
        self.maybe_free_model_hooks()
        if not return_dict:
            return frames
        return StableVideoDiffusionPipelineOutput(frames=frames)

    def _request_finish(self, latents, num_frames, decode_chunk_size, output_type):
        """final latents [R,F,4,h,w] -> what the caller receives: decode + frame export, or the latents themselves (output_type "latent")"""
        if output_type == "device":
            if not self.native_image_io:
                raise ValueError('output_type="device" needs a pipeline with native_image_io=True: the frames stay on the device as '
                                 "ops.frames_out writes them, and the torch request path has no such export")
            return self._frames_device(latents.to(self.vae.dtype), num_frames, decode_chunk_size)
        if self.native_image_io and output_type in ("np", "pil"):
            return self._frames_native(latents.to(self.vae.dtype), num_frames, decode_chunk_size, output_type)
        if output_type != "latent":
            return tensor2vid(self.decode_latents(latents.to(self.vae.dtype), num_frames, decode_chunk_size),
                              self.image_processor, output_type=output_type)
        return latents

    def _request_setup(self, image, condition_img, controlnet, prompt, use_text, text_encoder, height, width, num_frames,
                       num_inference_steps, min_guidance_scale, max_guidance_scale, fps, motion_bucket_id, noise_aug_strength,
                       num_videos_per_prompt, generator, latents, use_instructpix2pix, scheduler):
        """Everything step-invariant of a call's requests (reference :520-605): CLIP context, VAE image latents, gesture latents, time
        ids, the schedule of ``scheduler`` (set here), initial latents, the guidance ramp.  Shared by __call__ (the pipeline's
        scheduler) and by callers that serve a request on a scheduler instance of its own."""
        from types import SimpleNamespace
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        num_frames = num_frames if num_frames is not None else self.unet.config.num_frames
        self.check_inputs(image, height, width)
        batch_size = 1 if isinstance(image, PIL.Image.Image) else (len(image) if isinstance(image, list) else image.shape[0])
        nvid = 1 if num_videos_per_prompt is None else int(num_videos_per_prompt)
        if batch_size < 1 or nvid < 1:
            raise ValueError(f"need at least one image and one video per image, got {batch_size} image(s) x {nvid} video(s)")
        nreq = batch_size * nvid             # independent requests of this call, image-major: request i * nvid + j = video j of image i
        device = self._execution_device
        do_cfg = max_guidance_scale > 1.0

        ip2p = bool(use_instructpix2pix) and do_cfg
        if isinstance(generator, (list, tuple)) and len(generator) != nreq:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective "
                             f"batch size of {nreq} ({batch_size} image(s) x {nvid} video(s) per image). Make sure the batch size "
                             "matches the length of the generators.")
        lat_shape = (nreq, num_frames, self.unet.config.in_channels // 2, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is not None and tuple(latents.shape) != lat_shape:
            raise ValueError(f"latents {tuple(latents.shape)}: expected {lat_shape} = [{batch_size} image(s) x {nvid} video(s) per image, "
                             "F, 4, h, w]")
        cond = None
        if controlnet is not None:
            if isinstance(condition_img, GesturePoints) or (isinstance(condition_img, (list, tuple)) and len(condition_img) > 0
                                                            and all(isinstance(c, GesturePoints) for c in condition_img)):
                # the annotated points themselves: rasterised on the device straight to the fp16 that prepare_condition_image casts to
                # (quirk Q7) -- no host canvas and no copy of a map to the device
                cond = rasterise_points_device(condition_img, height, width, num_frames, device, torch.float16)
            else:
                cond = self.prepare_condition_image(condition_img, device)
            if cond.ndim not in (4, 5) or cond.shape[-4] != num_frames or (cond.ndim == 5 and cond.shape[0] != batch_size):
                raise ValueError(f"condition_img {tuple(cond.shape)}: expected [F,3,H,W] (shared by every request) or one [F,3,H,W] map per "
                                 f"image, [{batch_size},F,3,H,W], with F = {num_frames}")
        pixels = self._request_pixels(image, device)
        ehs = self.encode_clip(image if pixels is None else pixels, prompt, use_text, text_encoder, device, nvid, do_cfg, ip2p)
        if ehs.shape[0] != nreq * (1 if not do_cfg else 3 if ip2p else 2):
            raise ValueError(f"encode_clip returned {ehs.shape[0]} contexts for {nreq} request(s)")
        fps = fps - 1                                                            # SVD was conditioned on fps-1 (:527)
        upcast = self.vae.dtype == torch.float16 and getattr(self.vae.config, "force_upcast", False)
        if pixels is None:
            img = self.image_processor.preprocess(image, height=height, width=width)
            if nvid > 1:
                # every request noises its own copy of its image, as a call of its own would: generator r draws for request r.  (The
                # reference noises once per image and then tiles cat([neg, lat]) with repeat (:211-214), which pairs videos with the wrong class.)
                img = img.repeat_interleave(nvid, 0)
            img = img + noise_aug_strength * randn_tensor(img.shape, generator=generator, device=img.device, dtype=img.dtype)
        else:
            # the same draw as above -- same generator, shape, dtype and device of generation (a CPU or no generator draws on the host) --
            # handed to the kernel on the device; the kernel resizes, normalises, repeats each image for its videos (request r reads image
            # r // nvid), adds the noise and writes the dtype the VAE has inside the force_upcast window
            noise = randn_tensor((nreq, 3, height, width), generator=generator, device=torch.device("cpu") if generator is None else device,
                                 dtype=torch.float32).to(device)
            img = ops.vae_image(pixels.pixels, (height, width), noise, noise_aug_strength, torch.float32 if upcast else self.vae.dtype, nvid)
        if upcast:
            self.vae.to(dtype=torch.float32)
        # one image per request already: the CFG classes are concatenated around the R latents (class by class, the loop's order)
        image_latents = self._encode_vae_image(img.to(self.vae.dtype), device, 1, do_cfg, ip2p).to(ehs.dtype)
        image_latents = image_latents.unsqueeze(1).repeat(1, num_frames, 1, 1, 1)
        if upcast:
            self.vae.to(dtype=torch.float16)
        gesture_latents = None
        if controlnet is not None:
            # after the cast-back, in the VAE's own dtype: where (and in which precision) the reference encodes it (:652),
            # but once per request instead of once per step (loop-invariant, quirk Q6); one map per image: once per call
            gesture_latents = self._encode_gesture_maps(cond, nvid)
        added_time_ids = self._get_add_time_ids(fps, motion_bucket_id, noise_aug_strength, ehs.dtype, batch_size,
                                                nvid, do_cfg, use_instructpix2pix=ip2p).to(device)
        scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = scheduler.timesteps
        latents = self.prepare_latents(nreq, num_frames, self.unet.config.in_channels, height,
                                       width, ehs.dtype, device, generator, latents, scheduler=scheduler)
        guidance = torch.linspace(min_guidance_scale, max_guidance_scale, num_frames).unsqueeze(0).to(device, latents.dtype)
        guidance = append_dims(guidance.repeat(nreq, 1), latents.ndim)
        # which update the fused loop runs is the scheduler's to say: one with ``multistep_coefficients`` (DPMSolverMultistepScheduler) gets
        # the DPM-Solver++ 2M step kernel with those coefficients, any other the Euler step -- the loop never calls scheduler.step
        coefs = getattr(scheduler, "multistep_coefficients", None)
        return SimpleNamespace(sampler={} if coefs is None else {"multistep": coefs},nreq=nreq, num_frames=num_frames, height=height, width=width, do_cfg=do_cfg, ip2p=ip2p, ehs=ehs,
                               image_latents=image_latents, gesture_latents=gesture_latents, added_time_ids=added_time_ids,
                               timesteps=timesteps, sigmas=scheduler.sigmas, latents=latents, guidance=guidance)


class StableVideoDiffusionControlNetPipeline(_SVDPipelineCore):
    @torch.no_grad()
    def __call__(
        self,
        image: Union[PIL.Image.Image, List[PIL.Image.Image], torch.FloatTensor],
        condition_img: np.ndarray,
        controlnet: ControlNetModel,
        prompt=None,
        use_text: bool = False,
        text_encoder=None,
        height: int = 576,
        width: int = 1024,
        num_frames: Optional[int] = None,
        num_inference_steps: int = 25,
        min_guidance_scale: float = 1.0,
        max_guidance_scale: float = 3.0,
        fps: int = 7,
        motion_bucket_id: int = 127,
        noise_aug_strength: float = 0.02,
        decode_chunk_size: Optional[int] = None,
        num_videos_per_prompt: Optional[int] = 1,
        generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
        latents: Optional[torch.FloatTensor] = None,
        output_type: Optional[str] = "pil",
        callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
        callback_on_step_end_tensor_inputs: List[str] = ["latents"],
        return_dict: bool = True,
        controlnet_conditioning_scale: Union[float, List[float]] = 1.0,
        use_instructpix2pix: bool = False,
        control_guidance_start: Union[float, List[float]] = 0.0,
        control_guidance_end: Union[float, List[float]] = 1.0,
        inner_conditioning_scale: float = 1.0,
        guess_mode: bool = True,
        image_guidance_scale: float = 7.5,
    ):
        if not isinstance(controlnet, ControlNetModel):
            raise TypeError("controlnet must be a ControlNetModel")
        # the reference wraps both in a one-element list (:485-489), so only scalars work there; a one-element list
        # is accepted here as well
        if isinstance(control_guidance_start, (list, tuple)) or isinstance(control_guidance_end, (list, tuple)):
            if not (isinstance(control_guidance_start, (list, tuple)) and isinstance(control_guidance_end, (list, tuple))
                    and len(control_guidance_start) == len(control_guidance_end) == 1):
                raise ValueError("control_guidance_start/end: one value each (a single ControlNetModel)")
            control_guidance_start, control_guidance_end = control_guidance_start[0], control_guidance_end[0]
        if control_guidance_start >= control_guidance_end or control_guidance_start < 0.0 or control_guidance_end > 1.0:
            raise ValueError(f"control guidance window [{control_guidance_start}, {control_guidance_end}] must satisfy "
                             "0 <= start < end <= 1")
        if guess_mode and max_guidance_scale > 1.0:
            # reference :676-681 concatenates zeros onto residuals that already have the CFG batch, so the UNet's skip
            # additions fail on shape; test_code/inference.py always passes guess_mode=False.  Without CFG, guess_mode
            # only switches the 13 residual scales to logspace(-1, 0, 13) (temporal_controlnet.py:626-630): built.
            raise NotImplementedError("guess_mode=True with CFG cannot run in the reference either (:676-681); "
                                      "pass guess_mode=False as test_code/inference.py does")
        return self._generate(image, condition_img, controlnet, prompt, use_text, text_encoder, height, width, num_frames,
                              num_inference_steps, min_guidance_scale, max_guidance_scale, fps, motion_bucket_id,
                              noise_aug_strength, decode_chunk_size, num_videos_per_prompt, generator, latents, output_type,
                              callback_on_step_end, callback_on_step_end_tensor_inputs, return_dict,
                              controlnet_conditioning_scale, float(control_guidance_start), float(control_guidance_end),
                              use_instructpix2pix, image_guidance_scale, guess_mode)
