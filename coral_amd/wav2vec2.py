"""MI355X-native Wav2Vec2ForCTC engine (XLS-R family) behind CoRal's `model=wav2vec2-*` keys.

Host-side sequencing of the C-ABI kernels in libcoral_amd.so: forward, hand-written backward
and parameter/gradient storage.  It mirrors what `Wav2Vec2ForCTC.from_pretrained(...)` gives
CoRal (R/src/coral/wav2vec2.py:104-126): `model(input_values, attention_mask, labels)` ->
loss + logits ($TF/models/wav2vec2/modeling_wav2vec2.py:1667-1736), HF parameter names, CTC
with blank = pad id, reduction "sum", zero_infinity.

HBM layout
  * parameters: one flat fp32 master buffer + one flat fp32 gradient buffer + one flat bf16
    compute copy (same offsets), ordered [front | layer 0 | ... | layer L-1 | head] so that a
    data-parallel bucket is a contiguous slice (see coral_amd/trainer.py);
  * activations: channels-last [B*T, C] bf16; q,k,v of a layer live in one [B*T, 3d] matrix; the encoder
    layers are blocks.SelfAttnBlock + blocks.FFNBlock (fused attention, no [T, T] matrix in HBM);
  * conv layers 1..6 and the grouped positional conv run as implicit GEMMs over overlapping-row
    views (no im2col is ever materialised in the forward pass); they, the feature projection and the head are the blocks
    of stem_blocks.py;
  * packed mode (`pack_frames`): in a training step with labels the valid frames of the batch are laid
    end to end behind the positional conv, and the encoder layers, the final LayerNorm and lm_head run on those
    Mp = sum(flen) rows - a prefix of the same [B*T, C] buffers; logits and the gradient wrt h[0] return to [B, T, *].
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass

import torch

from . import ops
from .blocks import FFNBlock, Scratch, SelfAttnBlock, encoder_backward, wgrad_stream
from .engine import Engine
from .staging import PinnedStager
from .stem_blocks import ConvFeatureEncoder, FeatureProjection, LMHead, PosConvEmbed


@dataclass
class Wav2Vec2Shape:
    """Architecture hyper-parameters (HF Wav2Vec2Config subset used by XLS-R)."""

    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    intermediate_size: int = 4096
    conv_dim: tuple = (512,) * 7
    conv_kernel: tuple = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: tuple = (5, 2, 2, 2, 2, 2, 2)
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    vocab_size: int = 46
    pad_token_id: int = 45
    layer_norm_eps: float = 1e-5
    ctc_loss_reduction: str = "sum"
    ctc_zero_infinity: bool = True
    activation_dropout: float = 0.0
    layerdrop: float = 0.0
    # the other dropouts of Wav2Vec2Config ($TF/models/wav2vec2/modeling_wav2vec2.py:433,458,571,642,765,1698): training only,
    # scale 1 / (1 - p); Wav2Vec2CTCEngine.dropout_site gives every site its (p, seed)
    attention_dropout: float = 0.0
    hidden_dropout: float = 0.0
    feat_proj_dropout: float = 0.0
    final_dropout: float = 0.0

    @property
    def head_dim(self):
        return self.hidden_size // self.num_attention_heads


# CoRal model keys -> XLS-R shapes (R/config/model/wav2vec2-{small,medium,large}.yaml:3)
CORAL_W2V2_SHAPES = {
    "wav2vec2-small": dict(hidden_size=1024, num_hidden_layers=24, intermediate_size=4096),
    "wav2vec2-medium": dict(hidden_size=1280, num_hidden_layers=48, intermediate_size=5120),
    "wav2vec2-large": dict(hidden_size=1920, num_hidden_layers=48, intermediate_size=7680),
}


def _r8(n: int) -> int:
    return (n + 7) // 8 * 8


# The conv stack's pre-norm tensors (outputs of the conv GEMMs 1..6) and the last conv block's output stay fp32, as under
# the reference's autocast, where nn.LayerNorm and the GELU behind it run in fp32
# ($TF/models/wav2vec2/modeling_wav2vec2.py:291-298,429-434): 0.5 GB more at B = 8 and seven bf16 roundings less in front
# of the transformer.  CA_CONV_F32=0 restores the bf16 tensors (A/B measurements only).
CONV_F32 = os.environ.get("CA_CONV_F32", "1") == "1"


def frame_row_offsets(attention_mask: torch.Tensor, conv_kernel, conv_stride):
    """Host attention mask [B, N] -> (flen int64 [B], row_off int32 [B + 1]): the frames every utterance has behind the
    conv stack (`_get_feat_extract_output_lengths` of its sample count) and their cumulative sums, row_off[0] = 0 - where
    utterance b starts when the valid frames of the batch are laid end to end (row_off[B] = their number)."""
    n = attention_mask.to(torch.int64).sum(-1)
    for k, st in zip(conv_kernel, conv_stride):
        n = torch.div(n - k, st, rounding_mode="floor") + 1
    row_off = torch.zeros(n.numel() + 1, dtype=torch.int32)
    row_off[1:] = torch.cumsum(n, 0)
    return n, row_off


def _arena_build(build, device, default_dtype):
    """Run `build(z)` twice - z(n, dt=...) first only adds up 256-byte aligned sizes, then hands out views of one
    zero-filled arena - so that a workspace costs one allocation and one fill."""
    esz = {torch.bfloat16: 2, torch.float32: 4, torch.uint8: 1, torch.int32: 4}
    total = [0]

    def measure(n, dt=default_dtype):
        total[0] += (int(n) * esz[dt] + 255) // 256 * 256
        return None

    build(measure)
    arena = torch.zeros(total[0], dtype=torch.uint8, device=device)
    pos = [0]

    def carve(n, dt=default_dtype):
        nb = int(n) * esz[dt]
        v = arena[pos[0]:pos[0] + nb].view(dt)
        pos[0] += (nb + 255) // 256 * 256
        return v

    w = build(carve)
    w["_arena"] = arena
    return w


class ParamStore:
    """Flat fp32 master / fp32 grad / bf16 compute buffers with HF-named views."""

    def __init__(self, shapes: list[tuple[str, tuple, str]], device):
        self.index: dict[str, tuple[int, tuple]] = {}
        self.buckets: dict[str, list[int]] = {}
        off = 0
        for name, shape, bucket in shapes:
            n = int(math.prod(shape))
            self.index[name] = (off, tuple(shape))
            b = self.buckets.setdefault(bucket, [off, off])
            off += _r8(n)
            b[1] = off
        self.numel = off
        self.device = device
        self.p32 = torch.zeros(off, dtype=torch.float32, device=device)
        self.g32 = torch.zeros(off, dtype=torch.float32, device=device)
        self.p16 = torch.zeros(off, dtype=torch.bfloat16, device=device)
        self._g16 = None

    @property
    def g16(self) -> torch.Tensor:
        """bf16 gradient buffer with the same offsets (allocated on first use): the weight-matrix gradients of a step that
        does not accumulate stay bf16 - what the reference's autocast produces - from the weight-gradient GEMMs to AdamW
        (engine.wgrad_bf16, trainer.py)."""
        if self._g16 is None:
            self._g16 = torch.zeros(self.numel, dtype=torch.bfloat16, device=self.device)
        return self._g16

    def off(self, name: str) -> int:
        return self.index[name][0]

    def view(self, name: str, which: str = "p32") -> torch.Tensor:
        off, shape = self.index[name]
        n = int(math.prod(shape))
        buf = self.g16 if which == "g16" else vars(self)[which]  # (p32 / g32 / p16; g16 is allocated on first use)
        return buf[off:off + n].view(shape)

    def names(self):
        return list(self.index.keys())

    def refresh_bf16(self):
        ops.cast_f32_bf16(self.p32, self.p16, self.numel)


def w2v2_param_list(s: Wav2Vec2Shape) -> list[tuple[str, tuple, str]]:
    """(HF name, shape, bucket) in storage order; q/k/v of a layer are adjacent on purpose."""
    d, f = s.hidden_size, s.intermediate_size
    out = []
    cin = 1
    for i, (co, k) in enumerate(zip(s.conv_dim, s.conv_kernel)):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}."
        out += [(p + "conv.weight", (co, cin, k), "front"), (p + "conv.bias", (co,), "front"),
                (p + "layer_norm.weight", (co,), "front"), (p + "layer_norm.bias", (co,), "front")]
        cin = co
    K, G = s.num_conv_pos_embeddings, s.num_conv_pos_embedding_groups
    out += [
        ("wav2vec2.feature_projection.layer_norm.weight", (cin,), "front"),
        ("wav2vec2.feature_projection.layer_norm.bias", (cin,), "front"),
        ("wav2vec2.feature_projection.projection.weight", (d, cin), "front"),
        ("wav2vec2.feature_projection.projection.bias", (d,), "front"),
        ("wav2vec2.masked_spec_embed", (d,), "front"),
        ("wav2vec2.encoder.pos_conv_embed.conv.bias", (d,), "front"),
        ("wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original0", (1, 1, K), "front"),
        ("wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original1", (d, d // G, K), "front"),
    ]
    for l in range(s.num_hidden_layers):
        p = f"wav2vec2.encoder.layers.{l}."
        b = f"layer{l}"
        # small tensors first (one contiguous slice to clear per step), then the matrices whose
        # gradients are written -- not accumulated -- by the first micro-batch's wgrad GEMMs
        out += [(p + "layer_norm.weight", (d,), b), (p + "layer_norm.bias", (d,), b),
                (p + "final_layer_norm.weight", (d,), b), (p + "final_layer_norm.bias", (d,), b)]
        # the four Linear biases are contiguous (q|k|v, out, ffn1, ffn2 = 5d + f floats): their gradients come out of
        # the weight-gradient kernels as partial column sums and are added in one pass (backward())
        for n in ("q_proj", "k_proj", "v_proj"):
            out.append((p + f"attention.{n}.bias", (d,), b))
        out += [(p + "attention.out_proj.bias", (d,), b),
                (p + "feed_forward.intermediate_dense.bias", (f,), b),
                (p + "feed_forward.output_dense.bias", (d,), b)]
        for n in ("q_proj", "k_proj", "v_proj"):
            out.append((p + f"attention.{n}.weight", (d, d), b))
        out += [(p + "attention.out_proj.weight", (d, d), b),
                (p + "feed_forward.intermediate_dense.weight", (f, d), b),
                (p + "feed_forward.output_dense.weight", (d, f), b)]
    out += [("wav2vec2.encoder.layer_norm.weight", (d,), "head"),
            ("wav2vec2.encoder.layer_norm.bias", (d,), "head"),
            ("lm_head.weight", (s.vocab_size, d), "head"), ("lm_head.bias", (s.vocab_size,), "head")]
    return out


class CTCOutput(dict):
    """`model(**batch)` result: out["loss"], out.loss, out.logits (HF CausalLMOutput-like)."""

    __getattr__ = dict.get

    def __getitem__(self, k):
        if isinstance(k, int):
            return [self["loss"], self["logits"]][k] if self.get("loss") is not None else self["logits"]
        return dict.__getitem__(self, k)


DROPOUT_KEYS = ("activation_dropout", "attention_dropout", "hidden_dropout", "feat_proj_dropout", "final_dropout")

# dropout site -> (seed code, Wav2Vec2Shape field).  Sites of HF's stable-LayerNorm Wav2Vec2ForCTC:
#   feat_proj  after the feature projection, before SpecAugment / padding       ($TF/.../modeling_wav2vec2.py:433)
#   pos_conv   on h0 + pos_conv(h0) in front of layer 0 (the sum)               (:765)
#   attention  on the softmax probabilities of layer l                          (:458)
#   attn_out   on the attention output of layer l before its residual add       (:642)
#   ffn_out    on the FFN output of layer l before its residual add             (:571)
#   final      after the encoder's final LayerNorm, before lm_head              (:1698)
DROPOUT_SITES = {"attention": (1, "attention_dropout"), "attn_out": (2, "hidden_dropout"),
                 "ffn_out": (3, "hidden_dropout"), "feat_proj": (4, "feat_proj_dropout"),
                 "pos_conv": (5, "hidden_dropout"), "final": (6, "final_dropout")}


class Wav2Vec2CTCEngine(Engine):
    """Forward + backward of Wav2Vec2ForCTC as a fixed sequence of HIP kernels."""

    def __init__(self, shape: Wav2Vec2Shape, device="cuda:0", freeze_base: bool = False):
        site_p = [float(getattr(shape, k)) for k in {key for _, key in DROPOUT_SITES.values()}]
        if not all(0.0 <= v < 1.0 for v in site_p):
            raise ValueError(f"dropout probabilities must lie in [0, 1): {shape}")
        if shape.num_hidden_layers > 100 and any(site_p):
            raise ValueError("at most 100 encoder layers with dropout: the seeds of a step give every site a block of 100")
        self.s = shape
        self.device = torch.device(device)
        ops.lib()  # fail loudly if the HIP library is not built
        if not torch.cuda.is_available():
            raise ops.CoralAmdError("Wav2Vec2CTCEngine needs a GPU: there is no CPU path")
        s = shape
        assert s.hidden_size % 8 == 0 and (s.hidden_size // s.num_conv_pos_embedding_groups) % 8 == 0
        assert s.head_dim % 8 == 0
        self.store = ParamStore(w2v2_param_list(s), self.device)
        d = s.hidden_size
        self.feature_encoder = ConvFeatureEncoder(self.store, "wav2vec2.feature_extractor.conv_layers.", s.conv_dim,
                                                  s.conv_kernel, s.conv_stride, s.layer_norm_eps, CONV_F32)
        self.feature_projection = FeatureProjection(self.store, "wav2vec2.feature_projection.", s.conv_dim[-1], d,
                                                    s.layer_norm_eps)
        self.pos_conv = PosConvEmbed(self.store, "wav2vec2.encoder.pos_conv_embed.conv.", d, s.num_conv_pos_embedding_groups,
                                     s.num_conv_pos_embeddings)
        self.head = LMHead(self.store, "wav2vec2.encoder.layer_norm", "lm_head.weight", "lm_head.bias", d, s.vocab_size,
                           s.layer_norm_eps)
        self.blocks = []  # encoder layer l: (self-attention block, feed-forward block)
        for l in range(s.num_hidden_layers):
            p = f"wav2vec2.encoder.layers.{l}."
            self.blocks.append((
                SelfAttnBlock(self.store, p + "layer_norm", p + "attention.", s.num_attention_heads, s.hidden_size,
                              s.layer_norm_eps, False, p + "attention.q_proj.bias"),
                FFNBlock(self.store, p + "final_layer_norm", p + "feed_forward.intermediate_dense",
                         p + "feed_forward.output_dense", s.hidden_size, s.intermediate_size, s.layer_norm_eps)))
        self.freeze_base = freeze_base
        # packed mode (forward()): the encoder of a training step works on the valid frames only
        self.pack_frames = os.environ.get("CA_PACK_FRAMES", "0") not in ("", "0")
        self.last_rows = 0  # rows the encoder layers processed in the last forward: sum(flen) when packed, else B * T
        self.last_frames = 0  # ... and B * T of that forward
        self._ws = None
        self._ws_key = None
        self._ctc_key = None
        self._stager = PinnedStager(self.device)
        self._saved = None
        self.zero_embed = torch.zeros(d, dtype=torch.bfloat16, device=self.device)

    # ---- parameters ------------------------------------------------------------------------
    def load_state_dict(self, P: dict, strict: bool = True, seed: int = 4242, init_missing: bool = True) -> dict:
        """Copy HF-named fp32 tensors into the flat master buffer and refresh compute copies.

        strict=False follows `PreTrainedModel.from_pretrained` for the checkpoints CoRal finetunes from
        (R/src/coral/wav2vec2.py:107-126: a pretrained XLS-R base plus a freshly initialised CTC head): a bare
        `Wav2Vec2Model` state dict gets the `wav2vec2.` prefix, the pre-parametrize weight-norm names
        `...pos_conv_embed.conv.weight_g / weight_v` map to `parametrizations.weight.original0 / original1`,
        unexpected keys (`quantizer.*`, `project_q.*`, `project_hid.*` of the pretraining head) are ignored, and a
        missing or differently sized `lm_head.*` / `masked_spec_embed` is initialised from `seed` the way HF's
        `_init_weights` does (Linear: N(0, 0.02), zero bias; masked_spec_embed: U(0, 1)).  Anything else that is
        missing still raises; init_missing=False leaves the tolerated missing tensors as they are.  Returns {"missing": [...], "unexpected": [...]} like `load_state_dict` of torch."""
        if not strict:
            if not any(k.startswith("wav2vec2.") or k.startswith("lm_head.") for k in P):
                P = {"wav2vec2." + k: v for k, v in P.items()}
            ren = {}
            for k, v in P.items():
                if k.endswith("pos_conv_embed.conv.weight_g"):
                    k = k[:-len("weight_g")] + "parametrizations.weight.original0"
                elif k.endswith("pos_conv_embed.conv.weight_v"):
                    k = k[:-len("weight_v")] + "parametrizations.weight.original1"
                ren[k] = v
            P = ren
        names = self.store.names()
        fresh_ok = ("lm_head.weight", "lm_head.bias", "wav2vec2.masked_spec_embed")
        missing = [n for n in names if n not in P]
        if not strict:
            missing += [n for n in fresh_ok if n in P and int(P[n].numel()) != int(math.prod(self.store.index[n][1]))]
        hard = [n for n in missing if strict or n not in fresh_ok]
        if hard:
            raise KeyError(f"missing parameters: {hard[:4]}...")
        g = torch.Generator(device=self.device).manual_seed(seed)
        for n in names:
            v = self.store.view(n)
            if n in missing:
                if not init_missing:
                    continue  # keep the present value (resuming a run whose file follows HF's key set)
                if n == "lm_head.weight":
                    v.normal_(0.0, 0.02, generator=g)
                elif n == "lm_head.bias":
                    v.zero_()
                else:
                    v.uniform_(0.0, 1.0, generator=g)
                continue
            v.copy_(P[n].to(self.device, torch.float32).reshape(self.store.index[n][1]))
        self.refresh_compute_weights()
        return dict(missing=missing, unexpected=[k for k in P if k not in self.store.index])

    def state_dict(self) -> dict:
        return {n: self.store.view(n).detach().clone() for n in self.store.names()}

    def grad_dict(self) -> dict:
        return {n: self.store.view(n, "g32") for n in self.store.names()}

    # the four weight matrices of an encoder layer: (first parameter name, rows, columns)
    def _layer_matrices(self, l: int):
        d, f = self.s.hidden_size, self.s.intermediate_size
        pl = f"wav2vec2.encoder.layers.{l}."
        return [("qkv", pl + "attention.q_proj.weight", 3 * d, d), ("o", pl + "attention.out_proj.weight", d, d),
                ("fc1", pl + "feed_forward.intermediate_dense.weight", f, d),
                ("fc2", pl + "feed_forward.output_dense.weight", d, f)]

    def norm_matrices(self):
        """Every layer's weight matrices (>99 % of the buffer): the gradient norm needs no pass over them."""
        return [(l, *m) for l in range(self.s.num_hidden_layers) for m in self._layer_matrices(l)]

    def shard_ranges(self) -> dict:
        """{layer bucket: (first element of its weight matrices, bucket end)}: the part of every layer bucket a sharded
        optimiser (trainer.py, zero_stage) may split over the ranks - the forward reads these parameters through the
        bf16 compute copy only, the small tensors in front of them (LayerNorms, biases: read from the fp32 master) stay
        replicated."""
        st = self.store
        return {f"layer{l}": (st.off(f"wav2vec2.encoder.layers.{l}.attention.q_proj.weight"), st.buckets[f"layer{l}"][1])
                for l in range(self.s.num_hidden_layers)}

    def bf16_grad_ranges(self) -> dict:
        """{layer bucket: (lo, hi)}: the weight matrices whose gradients a single-micro-batch step may keep in bf16
        (trainer.py, ParamStore.g16): every layer's, = shard_ranges()."""
        return self.shard_ranges()

    def zero_grad(self, matrices: bool = True):
        """Clear gradients.  matrices=False clears everything except the transformer layers' weight
        matrices (>99 % of the bytes): the next backward(overwrite_matrices=True) writes those
        instead of accumulating, which saves a full read + write of the gradient buffer."""
        st = self.store
        if matrices:
            st.g32.zero_()
            self.pre_zeroed = False
            return
        if self.pre_zeroed:
            # the trainer already cleared these slices on its optimiser stream, right behind the AdamW launches that
            # consumed them (hidden under the forward instead of sitting in front of the backward)
            self.pre_zeroed = False
            return
        self.clear_small_grads()

    preclear_small_grads = True

    def clear_small_grads(self):
        """Zero everything except the transformer layers' weight matrices (see zero_grad): the front and head
        buckets and every layer's small tensors (LayerNorms, biases), as ONE launch over a cached range table."""
        st = self.store
        if self._small_ranges is None:
            rs = [(lo, hi - lo) for lo, hi in (st.buckets[n] for n in ("front", "head"))]
            for l in range(self.s.num_hidden_layers):
                lo = st.off(f"wav2vec2.encoder.layers.{l}.layer_norm.weight")
                rs.append((lo, st.off(f"wav2vec2.encoder.layers.{l}.attention.q_proj.weight") - lo))
            self._small_ranges = tuple(rs)
        ops.clear_ranges(st.g32, self._small_ranges)

    def dropout_site(self, site: str, l: int = 0, training: bool | None = None) -> tuple:
        """(p, seed) of one dropout site (DROPOUT_SITES) of layer l in the current step; (0.0, 0) outside training or
        with p = 0.  The forward and the backward both ask here, so the backward regenerates the forward's masks.

        Seeds: step_seed * 1000 + 100 * code + l.  The activation dropout of layer l keeps step_seed * 1000 + l, so the
        sites and layers of one step draw from disjoint seeds (l < 100), and no seed of one step is one of another."""
        code, key = DROPOUT_SITES[site]
        shape = self.s
        p = float(getattr(shape, key)) if (self.training if training is None else training) else 0.0
        if p <= 0.0:
            return 0.0, 0
        return p, self.step_seed * 1000 + 100 * code + l

    def refresh_compute_weights(self):
        """fp32 masters -> bf16 copies, conv weight reorders, weight-normed pos-conv weights."""
        self.store.refresh_bf16()
        self.refresh_derived()

    # the derived weights in the order the forward needs them: the trainer records one event per part, so the conv
    # stack does not wait for the weight-normed positional conv to be rebuilt (_await("front_posconv"))
    derived_parts = ("conv", "posconv")

    def refresh_derived(self, part: str | None = None):
        """Weights whose compute copy is not a plain cast (after an optimiser step the flat bf16
        copy is already written by ca_adamw_step).  part: None = all, or one of `derived_parts`."""
        if part in (None, "conv"):
            self.feature_encoder.refresh()
        if part in (None, "posconv"):
            self.pos_conv.refresh()

    # ---- shapes / workspaces -------------------------------------------------------------------
    def conv_lengths(self, N: int) -> list[int]:
        out, n = [], N
        for k, st in zip(self.s.conv_kernel, self.s.conv_stride):
            n = (n - k) // st + 1
            out.append(n)
        return out

    def feat_lengths(self, sample_lengths: torch.Tensor) -> torch.Tensor:
        n = sample_lengths.clone().long()
        for k, st in zip(self.s.conv_kernel, self.s.conv_stride):
            n = torch.div(n - k, st, rounding_mode="floor") + 1
        return n

    def _workspace(self, B: int, N: int):
        key = (B, N)
        if self._ws_key == key:
            return self._ws
        s, dev = self.s, self.device
        d, f = s.hidden_size, s.intermediate_size
        L = s.num_hidden_layers
        Ts = self.conv_lengths(N)
        T = Ts[-1]
        M = B * T
        bf, f32 = torch.bfloat16, torch.float32

        def build(z):
            # (run twice: once to measure, once to carve views out of ONE zero-filled arena - a workspace used to
            # be ~450 separate torch.zeros fills)
            w = {"B": B, "N": N, "Ts": Ts, "T": T, "M": M}
            pf = max(
                ops.layernorm_bwd_partial_floats(B * Ts[1], 512), ops.layernorm_bwd_partial_floats(M, d),
                ops.colsum_partial_floats(M, max(f, 3 * d)), ops.colsum_partial_floats(B * Ts[1], 512),
                ops.conv0_bwd_partial_floats(B, N, s.conv_dim[0], s.conv_kernel[0], s.conv_stride[0]), 4096)
            w["partial"] = z(pf, dt=f32)
            # the blocks' saved activations and backward scratch (stem_blocks.py, blocks.py)
            w["fe"] = self.feature_encoder.alloc(B, Ts, z, w["partial"])
            w["fp"] = self.feature_projection.alloc(M, z)
            w["h0"] = z(M * d)
            w["pc"] = self.pos_conv.alloc(B, T, z)
            w["h"] = [z(M * d) for _ in range(L + 1)]      # residual stream entering layer l (h[L] = out)
            w["hpk"] = z(M * d)                            # packed mode: the valid rows of h[0], laid end to end
            w["h1"] = [z(M * d) for _ in range(L)]         # ... between layer l's attention and feed-forward blocks
            w["sv"] = [(sa.alloc(B, T, z), ff.alloc(M, z)) for sa, ff in self.blocks]
            w["head"] = self.head.alloc(M, z)
            Vp = w["Vp"] = self.head.Vp
            w["logits"] = z(M * Vp, dt=f32)
            w["dlogits"] = z(M * Vp, dt=f32)
            w["dlogits16"] = z(M * Vp)
            w["dlogits16p"] = z(M * Vp)                    # packed mode: the valid rows of dlogits16
            w["nll"] = z(B, dt=f32)
            # backward scratch
            w["dA"] = z(M * d)
            # the encoder layers' (blocks.encoder_backward): gradients wrt the residual stream and, with hidden dropout, their
            # masked copies (the second outputs of the LayerNorm backwards), two sets of layer scratch and of fused
            # bias-gradient partials - what a layer's weight gradients read on their own stream stays intact for two layers
            w["ring"] = [z(M * d) for _ in range(6)]
            w["mring"] = [z(M * d) for _ in range(6)] if s.hidden_dropout > 0 else None
            w["scs"] = [Scratch(M, d, f, z, masks=False) for _ in range(2)]
            # (partial column sums of the layer's four dY: rows that a problem with fewer than COLSUM_PARTS tile columns
            # never writes stay zero)
            w["bias_ws"] = [z(ops.COLSUM_PARTS * (5 * d + f), dt=f32) for _ in range(2)]
            # LayerNorm-backward partials (d gamma | d beta per row block) of a layer's two norms, two layers in flight
            w["ln_partial"] = [[z(ops.layernorm_bwd_partial_floats(M, d), dt=f32) for _ in range(2)] for _ in range(2)]
            return w

        w = _arena_build(build, dev, bf)
        self._ws, self._ws_key = w, key
        return w

    # ---- forward -------------------------------------------------------------------------------
    def __call__(self, input_values, attention_mask=None, labels=None, mask_time=None,
                 mask_feature=None, layer_keep=None):
        return self.forward(input_values, attention_mask, labels, mask_time, mask_feature, layer_keep)

    def forward(self, input_values, attention_mask=None, labels=None, mask_time=None,
                mask_feature=None, layer_keep=None) -> CTCOutput:
        """input_values f32 [B,N] (already zero-mean/unit-var: the reference's feature extractor
        output), attention_mask [B,N] or None, labels i64/i32 [B,L] (-100 padded) or None.

        Packed mode: with `pack_frames` set, in training mode, with labels and at least one padded frame in the batch,
        the rows behind the positional conv are the valid frames only (`last_rows` = their number Mp < B * T): the
        `pos_conv` dropout site still draws on the [B, T, d] layout, then h[0] is packed, the layers, the final LayerNorm,
        the `final` dropout and lm_head run on Mp rows and the logits are scattered back into [B, T, V] (frames at or past
        an utterance's length hold 0; unpacked they hold what the padding computes - CTC reads neither).  Loss and
        gradients are those of the unpacked step up to rounding: a padded frame is never a key, never reaches the loss
        and so carries no gradient.  The elementwise dropout sites inside the packed region (attn_out, ffn_out, final,
        activation dropout) hash the packed flat index - another, equally valid draw than the unpacked step's; the
        attention-probability masks are the unpacked step's.  The row offsets are built on the host from the
        attention mask (the collator's host tensor: no extra transfer beyond staging B + 1 integers); a mask that
        already lives on the device costs one B-integer device-to-host copy, which waits for the stream.  Evaluation
        forwards, forwards without labels and full batches take the unpacked launches, bit for bit."""
        s, st = self.s, self.store
        dev = self.device
        x = self._stager.to_device(input_values, torch.float32, "x")
        B, N = x.shape
        w = self._workspace(B, N)
        d = s.hidden_size
        L = s.num_hidden_layers
        T, M, Vp = w["T"], w["M"], w["Vp"]

        if attention_mask is not None:
            am = self._stager.to_device(attention_mask, torch.int32, "am")
            flen = torch.empty(B, dtype=torch.int32, device=dev)
            ops.frame_lengths(am, s.conv_kernel, s.conv_stride, flen)
        else:
            if w.get("flen_full") is None:  # (cached: no fill kernel per step)
                w["flen_full"] = torch.full((B,), T, dtype=torch.int32, device=dev)
            flen = w["flen_full"]
        keep = [True] * L if layer_keep is None else list(layer_keep)
        w["flen"] = flen
        rows = None  # packed mode: (row_off int32 [B + 1] on the device, Mp)
        if self.pack_frames and self.training and labels is not None and attention_mask is not None:
            if attention_mask.device.type == "cpu":
                fl, row_off = frame_row_offsets(attention_mask, s.conv_kernel, s.conv_stride)
            else:  # (the B-integer device-to-host copy: the frame lengths the kernel above just produced)
                fl = flen.cpu().to(torch.int64)
                row_off = torch.zeros(B + 1, dtype=torch.int32)
                row_off[1:] = torch.cumsum(fl, 0)
            Mp = int(row_off[B])
            # (an utterance without a frame, or lengths beyond T, are not this path's business; Mp == M: nothing to drop,
            # and the attention kernels' tile loads are promised rows behind Mp inside the buffers)
            if int(fl.min()) >= 1 and int(fl.max()) <= T and Mp < M:
                rows = (self._stager.to_device(row_off, torch.int32, "row_off"), Mp)
        Me = M if rows is None else rows[1]  # rows of the encoder layers and the head
        kw_rows = {} if rows is None else dict(rows=rows)
        self.last_rows, self.last_frames = Me, M
        self._await("front")

        feats = self.feature_encoder.forward(x, w["fe"], B, N)
        self.feature_projection.forward(feats, w["h0"], w["fp"], M, self.dropout_site("feat_proj"))
        # SpecAugment + padding
        # (host-sampled masks and labels go through pinned staging: a pageable .to(device) here would stall the host
        # until the GPU had drained the previous step)
        tm = self._stager.to_device(mask_time, torch.uint8, "tm") if mask_time is not None else None
        fm = self._stager.to_device(mask_feature, torch.uint8, "fm") if mask_feature is not None else None
        ops.mask_frames(w["h0"], tm, fm, st.p16[st.off("wav2vec2.masked_spec_embed"):], flen, B, T, d)
        # positional conv embedding: h = h0 + gelu(conv(h0) + b)
        self._await("front_posconv")
        self.pos_conv.forward(w["h0"], w["h"][0], w["pc"], B, T)
        pa = self.dropout_site("pos_conv")
        if pa[0] > 0:  # (hidden dropout on the sum h0 + pos_conv(h0): layer 0 and its LN backward read the dropped values)
            ops.dropout(w["h"][0], w["h"][0], M * d, *pa)
        hs = w["h"]
        if rows is not None:
            ops.pack_rows(w["h"][0], w["hpk"], rows[0], B, T, d)
            hs = [w["hpk"]] + w["h"][1:]
        # encoder layers
        drop_p = s.activation_dropout if self.training else 0.0
        for l, (sa, ff) in enumerate(self.blocks):
            hin, hout = hs[l], hs[l + 1]
            if not keep[l]:
                hout[:Me * d].copy_(hin[:Me * d])
                continue
            self._await(f"layer{l}")
            sv_a, sv_f = w["sv"][l]
            sa.forward(hin, w["h1"][l], sv_a, B, T, klen=flen, hdrop=self.dropout_site("attn_out", l),
                       adrop=self.dropout_site("attention", l), **kw_rows)
            ff.forward(w["h1"][l], hout, sv_f, Me, drop_p, self.step_seed * 1000 + l, hdrop=self.dropout_site("ffn_out", l))
        # final LN + lm_head (fp32 logits, ld = Vp)
        self._await("head")
        for l in range(L):  # dropped layers were not waited for above; the backward reads every layer's weights
            if not keep[l]:
                self._await(f"layer{l}")
        V = s.vocab_size
        # (packed: the Mp logit rows land in the dlogits buffer - CTC writes it only afterwards - and are scattered from
        # there into the [B, T, Vp] buffer CTC and the caller read, zeros in the padded frames)
        self.head.forward(hs[L], w["head"], Me, logits=w["logits"] if rows is None else w["dlogits"],
                          drop=self.dropout_site("final"))
        if rows is not None:
            ops.unpack_rows(w["dlogits"], w["logits"], rows[0], B, T, Vp)
        logits = w["logits"].view(B, T, Vp)[:, :, :V]
        out = CTCOutput(logits=logits, loss=None)
        self._saved = dict(w=w, x=x, flen=flen, keep=keep, tm=tm, fm=fm, B=B, N=N,
                           has_loss=False, training=self.training, rows=rows, hs=hs)
        if labels is not None:
            lab = self._stager.to_device(labels, torch.int32, "lab")
            Lmax = lab.shape[1]
            in_len = flen
            key = (B, T, Lmax)
            if self._ctc_key != key:
                self._ctc_ws = torch.zeros(ops.ctc_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=dev)
                self._ctc_key = key
            gscale = None
            if s.ctc_loss_reduction == "mean":
                tl = (lab >= 0).sum(-1).clamp(min=1).to(torch.float32)
                gscale = (1.0 / (tl * B)).contiguous()
            ops.ctc_loss_fwd_bwd(w["logits"], lab, in_len, w["nll"], w["dlogits"], gscale, self._ctc_ws,
                                 B, T, V, Vp, Lmax, s.pad_token_id, s.ctc_zero_infinity)
            nll = w["nll"]
            out["nll"] = nll
            out["loss"] = nll.sum() if gscale is None else (nll * gscale).sum()
            self._saved["has_loss"] = True
        return out

    # ---- backward ------------------------------------------------------------------------------
    def backward(self, loss_scale: float = 1.0, overwrite_matrices: bool = False, bucket_done=None):
        """Back-propagate d(loss*loss_scale) into the flat gradient buffer (+=).

        bucket_done(name): called as soon as every gradient of a parameter bucket ("head",
        "layer{l}" in reverse order, "front") has been enqueued — the data-parallel trainer
        starts that bucket's all-reduce on its communication stream from this hook."""
        done = bucket_done if bucket_done is not None else (lambda name: None)
        sv = self._saved
        if sv is None or not sv["has_loss"]:
            raise RuntimeError("backward() needs a forward pass with labels")
        s, st = self.s, self.store
        w, x, flen, keep = sv["w"], sv["x"], sv["flen"], sv["keep"]
        B, N = sv["B"], sv["N"]
        d = s.hidden_size
        L = s.num_hidden_layers
        T, M, Vp = w["T"], w["M"], w["Vp"]
        part = w["partial"]
        # small tensors, front and head always accumulate (zero_grad clears them)
        lacc = not overwrite_matrices  # layer weight matrices: accumulate or overwrite
        # ... and, when they are overwritten (one micro-batch per optimiser step) and the trainer asked for it, kept in
        # bf16: the reference's autocast computes a Linear's weight gradient as a bf16 matmul output and only casts it to
        # fp32 when it lands in .grad.  Halves the store of the step's dominant kernel and the optimiser's gradient read.
        self.matrix_grads_bf16 = bool(overwrite_matrices and self.wgrad_bf16)
        gm = st.g16 if self.matrix_grads_bf16 else st.g32

        # head: dlogits (fp32) -> bf16 for the MFMA path
        dl = w["dlogits"]
        if isinstance(loss_scale, torch.Tensor):  # autograd route: the incoming gradient stays on the device
            ops.wave_scale(dl, loss_scale.reshape(1).to(torch.float32), dl, 1, M * Vp)
        elif loss_scale != 1.0:
            ops.wave_scale(dl, self._scale_scalar(loss_scale), dl, 1, M * Vp)
        ops.cast_f32_bf16(dl, w["dlogits16"], M * Vp)
        d16 = w["dlogits16"]
        # packed mode: the head and the encoder layers on the forward's Mp valid rows (Me), the rest on [B, T]
        rows, hs = sv["rows"], sv["hs"]
        Me = M if rows is None else rows[1]
        if rows is not None:
            ops.pack_rows(d16, w["dlogits16p"], rows[0], B, T, Vp)
            d16 = w["dlogits16p"]
        tr = sv["training"]

        def branch_site(j):
            """(p, seed) of the hidden dropout whose output the residual stream h[j] carries: the FFN-output site of the
            highest kept layer below j, or the one on h0 + pos_conv(h0) when there is none (dropped layers are the
            identity and draw no masks)."""
            below = [k for k in range(j) if keep[k]]
            if not below and rows is not None:
                # packed: the pos_conv site drew on [B, T, d] - its mask meets the gradient after the unpack below
                return 0.0, 0
            return self.dropout_site("ffn_out", below[-1], tr) if below else self.dropout_site("pos_conv", training=tr)

        ring, mring = w["ring"], w["mring"]
        # ring[0]: the gradient wrt the residual stream leaving layer L-1; mring[0]: dropout(ring[0]) with the mask of the
        # hidden-dropout site whose output that stream carries - the gradient of that site's branch
        drop = branch_site(L)
        self.head.backward(d16, hs[L], w["dA"], ring[0], w["head"], Me, part, freeze=self.freeze_base,
                           drop=self.dropout_site("final", training=tr), xdrop=(*drop, mring[0]) if drop[0] > 0 else None)
        done("head")
        if self.freeze_base:
            return
        # Weight gradients on their own stream: dW = dY^T X feeds only the optimiser, so a layer's weight-gradient launch
        # (MFMA-bound, 256x256 tiles, one workgroup per CU) runs beside the NEXT layer's data-gradient chain (128x128-tile
        # GEMMs, attention backward, LayerNorm backward: VALU / HBM-bound kernels and GEMM tails that leave matrix pipes
        # idle); it goes out as soon as the layer's attention backward has produced its last dY.
        dh, dhm, dpc = encoder_backward(
            self.blocks, w["sv"], keep, B, T, ring, w["scs"], w["bias_ws"], w["ln_partial"], gm=gm, acc=lacc,
            plan=self.norm_plan(), names=[f"layer{l}" for l in range(L)], side=wgrad_stream(self), wgrad_early=True,
            matrix_range=lambda l: self.shard_ranges()[f"layer{l}"], done=done, below=branch_site, mring=mring,
            **({} if rows is None else dict(rows=rows)))
        # dh: gradient wrt h[0] = h0m + gelu(pc_pre)
        # (hidden dropout on h0 + pos_conv(h0): both terms see the masked gradient)
        dg = dhm if branch_site(0)[0] > 0 else dh
        if rows is not None:
            # back to [B, T, d] (zeros in the padded frames) in a ring buffer nothing uses any more, then the pos_conv
            # site's mask
            dg = next(r for r in ring if r is not dh and r is not dpc)
            ops.unpack_rows(dh, dg, rows[0], B, T, d)
            pc = self.dropout_site("pos_conv", training=tr)
            if pc[0] > 0:
                ops.dropout(dg, dg, M * d, *pc)
        dh0 = w["dA"]
        self.pos_conv.backward(dg, dpc, dh0, w["pc"], B, T, part)
        # SpecAugment / padding backward: masked rows feed masked_spec_embed, then are zeroed
        if sv["tm"] is not None:
            ops.colsum(dh0, d, M, d, st.g32, part, rowmask=sv["tm"], out_off=st.off("wav2vec2.masked_spec_embed"))
        ops.mask_frames(dh0, sv["tm"], sv["fm"], self.zero_embed, flen, B, T, d)
        # (the projection's output was dropped before SpecAugment / padding)
        fe = w["fe"]
        self.feature_projection.backward(dh0, fe["a"][-1], fe["dy"], fe["dconv"][-1], w["fp"], M, part,
                                         self.dropout_site("feat_proj", training=tr))
        self.feature_encoder.backward(x, fe, B, N)
        done("front")

    def _scale_scalar(self, v: float) -> torch.Tensor:
        """A device scalar holding `v` (cached per value: 1/accum, no fill kernel per step)."""
        cache = self.__dict__.setdefault("_scalars", {})
        t = cache.get(v)
        if t is None:
            if len(cache) > 64:
                cache.clear()
            t = cache[v] = torch.full((1,), float(v), dtype=torch.float32, device=self.device)
        return t

    # ---- inference helpers -----------------------------------------------------------------------
    def greedy_decode(self, logits_full: torch.Tensor | None = None, in_len=None):
        """argmax + collapse + drop blank on the logits of the last forward (ids list per row)."""
        sv = self._saved
        w = sv["w"]
        B, T, V, Vp = sv["B"], w["T"], self.s.vocab_size, w["Vp"]
        dev = self.device
        raw = torch.empty(B, T, dtype=torch.int32, device=dev)
        ids = torch.empty(B, T, dtype=torch.int32, device=dev)
        olen = torch.empty(B, dtype=torch.int32, device=dev)
        ops.ctc_greedy_decode(w["logits"], in_len, raw, ids, olen, B, T, V, Vp, self.s.pad_token_id)
        ids_c, olen_c = ids.cpu(), olen.cpu()
        return [ids_c[b, :int(olen_c[b])].tolist() for b in range(B)], raw

    def beam_decode(self, lm=None, beam_width: int = 100, in_len=None, tokenizer=None, logits=None, n_best: int = 1,
                    hotwords=None, hotword_weight: float = 10.0, **params):
        """CTC prefix beam search on the logits of the last forward, fused with the n-gram LM `lm` (the device-table
        dict of `NGramLM.device_tables`, or an `NGramLM` together with `tokenizer`; None: no LM, for which
        alpha = beta = 0 is the plain CTC prefix beam search).  `params`: alpha, beta, unk_score_offset,
        token_min_logp, beam_prune_logp, score_boundary (defaults: coral_amd/ngram.py).  `tokenizer` names the word
        delimiter and the ids that are never emitted (<s>, </s>, <unk>); without it there are no word boundaries and
        nothing is forbidden.  `logits`: a contiguous fp32 device tensor [B, T, ld >= V] to decode instead of the last
        forward's (the stitched rows of coral_amd/longform.py).
        -> (ids list per row, scores fp32 [B] = S(y)).
        n_best > 1 or hotwords other than None (a list of words or phrases, or the dict of `ngram.hotword_tables`; each word that closes
        adds hotword_weight) go through `ca_ctc_beam_decode_ex` and return, per row, a list of at most
        n_best {"ids", "score", "logit_score", "lm_score"}, best first; hotwords need `tokenizer`, with or without an LM.
        An empty hotword list or hotword_weight = 0 is "no hotwords"."""
        from .ngram import DEFAULT_PARAMS, hotword_tables

        V = self.s.vocab_size
        dev = self.device
        if logits is None:
            sv = self._saved
            w = sv["w"]
            B, T, Vp = sv["B"], w["T"], w["Vp"]
            logits = w["logits"]
        else:
            if (logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.shape[2] < V
                    or not logits.is_cuda):
                raise ValueError("beam_decode: logits must be a contiguous fp32 [B, T, ld >= V] tensor on the engine's device")
            B, T, Vp = logits.shape
        blank = self.s.pad_token_id
        if tokenizer is not None:
            delim = tokenizer.vocab[tokenizer.word_delimiter_token]
            never = [tokenizer.bos_token_id, tokenizer.eos_token_id, tokenizer.unk_token_id]
        else:
            delim, never = -1, []
        if lm is not None and not isinstance(lm, dict):
            if tokenizer is None:
                raise ValueError("beam_decode: an NGramLM needs the tokenizer that spells its words")
            lm = lm.device_tables(tokenizer, dev)
        if lm is not None and delim < 0:
            raise ValueError("beam_decode: LM fusion needs the tokenizer (word delimiter id)")
        unknown = set(params) - set(DEFAULT_PARAMS)
        if unknown:
            raise TypeError(f"beam_decode: unknown parameters {sorted(unknown)}")
        p = dict(DEFAULT_PARAMS, **params)
        if not isinstance(n_best, int) or isinstance(n_best, bool) or not 1 <= n_best <= beam_width:
            raise ValueError(f"beam_decode: n_best={n_best!r} must be an integer in 1..beam_width = {beam_width}")
        if not isinstance(hotword_weight, (int, float)) or not math.isfinite(hotword_weight):
            raise ValueError(f"beam_decode: hotword_weight={hotword_weight!r} must be a finite number")
        extended = n_best != 1 or hotwords is not None  # what decides the return type: the arguments, not their values
        if hotwords is not None and not isinstance(hotwords, dict):
            if tokenizer is None:
                raise ValueError("beam_decode: hotwords need the tokenizer that spells them (and names the word delimiter)")
            hotwords = hotword_tables(hotwords, tokenizer, dev)
        if hotwords is not None and (hotwords["hot_keys"].numel() == 0 or hotword_weight == 0):
            hotwords = None
        if hotwords is not None and delim < 0:
            raise ValueError("beam_decode: hotwords need the tokenizer (word delimiter id)")
        forbidden = torch.zeros(V, dtype=torch.uint8)
        for i in never:
            if 0 <= i < V and i != blank:
                forbidden[i] = 1
        if extended:
            ids = torch.empty(B, n_best, T, dtype=torch.int32, device=dev)
            olen = torch.empty(B, n_best, dtype=torch.int32, device=dev)
            split = torch.empty(3, B, n_best, dtype=torch.float32, device=dev)
            n_out = torch.empty(B, dtype=torch.int32, device=dev)
            ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, V, beam_width), dtype=torch.uint8, device=dev)
            ops.ctc_beam_decode_ex(logits, in_len, ids, olen, split[0], split[1], split[2], n_out, ws, B, T, V, Vp, blank,
                                   delim, forbidden.to(dev), lm, n_best=n_best, hotwords=hotwords,
                                   hotword_weight=float(hotword_weight), beam_width=beam_width, **p)
            ids_c, olen_c, split_c, n_c = ids.cpu(), olen.cpu(), split.cpu(), n_out.cpu()
            return [[dict(ids=ids_c[b, r, :int(olen_c[b, r])].tolist(), score=float(split_c[0, b, r]),
                          logit_score=float(split_c[1, b, r]), lm_score=float(split_c[2, b, r]))
                     for r in range(int(n_c[b]))] for b in range(B)]
        ids = torch.empty(B, T, dtype=torch.int32, device=dev)
        olen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.ctc_beam_workspace_bytes(B, T, V, beam_width), dtype=torch.uint8, device=dev)
        ops.ctc_beam_decode(logits, in_len, ids, olen, score, ws, B, T, V, Vp, blank, delim, forbidden.to(dev), lm,
                            beam_width=beam_width, **p)
        ids_c, olen_c = ids.cpu(), olen.cpu()
        return [ids_c[b, :int(olen_c[b])].tolist() for b in range(B)], score

    def align(self, labels, in_len=None, logits=None):
        """CTC forced alignment (ca_ctc_align) of one id list per row to the logits of the last forward, or to
        `logits`, a contiguous fp32 device tensor [B, T, ld >= V] (the stitched rows of coral_amd/longform.py).  The ids
        lie in [0, V) and differ from the blank (= pad) id; at most CA_CTC_ALIGN_MAX_LABELS of them per row.
        -> (rows, score): per row the host lists (start, end, tok_score) - a token's first frame on the most probable
        alignment, the first frame behind its last one, the mean log-probability of its frames - and the alignments'
        log-probabilities as a host list; a row that has no alignment has score -inf and start = end = -1.  One
        device-to-host copy."""
        V = self.s.vocab_size
        dev = self.device
        if logits is None:
            sv = self._saved
            w = sv["w"]
            B, T, Vp = sv["B"], w["T"], w["Vp"]
            logits = w["logits"]
        else:
            if (logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.shape[2] < V
                    or not logits.is_cuda):
                raise ValueError("align: logits must be a contiguous fp32 [B, T, ld >= V] tensor on the engine's device")
            B, T, Vp = logits.shape
        labels = [list(map(int, r)) for r in labels]
        if len(labels) != B:
            raise ValueError(f"align: {len(labels)} label rows for {B} rows of logits")
        Lmax = max([len(r) for r in labels] + [1])
        lab = torch.zeros(B, Lmax, dtype=torch.int32)
        for b, r in enumerate(labels):
            lab[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
        lab_len = torch.tensor([len(r) for r in labels], dtype=torch.int32)
        # start | end | tok_score bits | score bits in one int32 buffer: one copy to the host
        out = torch.empty(3 * B * Lmax + B, dtype=torch.int32, device=dev)
        start, end = out[:B * Lmax].view(B, Lmax), out[B * Lmax:2 * B * Lmax].view(B, Lmax)
        tok = out[2 * B * Lmax:3 * B * Lmax].view(torch.float32).view(B, Lmax)
        score = out[3 * B * Lmax:].view(torch.float32)
        ws = torch.empty(max(1, ops.ctc_align_workspace_bytes(B, T, Lmax)), dtype=torch.uint8, device=dev)
        ops.ctc_align(logits, in_len, lab, lab_len, start, end, tok, score, ws, B, T, V, Vp, Lmax, self.s.pad_token_id)
        host = out.cpu()
        h = host[:2 * B * Lmax].view(2, B, Lmax)
        ht = host[2 * B * Lmax:3 * B * Lmax].view(torch.float32).view(B, Lmax)
        rows = [(h[0, b, :len(r)].tolist(), h[1, b, :len(r)].tolist(), ht[b, :len(r)].tolist())
                for b, r in enumerate(labels)]
        return rows, host[3 * B * Lmax:].view(torch.float32).tolist()
