"""CPU: the attention-map entry points refuse bad arguments through the ABI without touching a GPU, and the reference that the GPU
tests hold get_last_selfattention / get_intermediate_layers to (vit.pyc@L255-272) is pinned against an independent
implementation, a locally configured HF ViTModel (eager attention, no download)."""
import ctypes

import pytest
import torch

from oracle import vit_oracle as vo


def reference_attention_and_layers(p, x, arch):
    """The reference's two inference methods composed from the oracle's primitives: (softmax attention of the last block
    [B, H, N, N], [norm(x) after block i for every block i]) -- get_intermediate_layers(x, n) is the last n of the list."""
    a = vo.ARCHS[arch]
    depth, H = a["depth"], a["num_heads"]
    t = vo.prepare_tokens(x, p)
    layers = []
    for i in range(depth):
        if i == depth - 1:      # Attention.forward up to the softmax (vit.pyc@L119-131), return_attention=True (L146-152)
            b = f"blocks.{i}."
            h = vo.layer_norm(t, p[b + "norm1.weight"], p[b + "norm1.bias"])
            B, N, C = h.shape
            qkv = (h @ p[b + "attn.qkv.weight"].t() + p[b + "attn.qkv.bias"]).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
            attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * (C // H) ** -0.5).softmax(dim=-1)
        t = vo.block(t, p, i, H)
        layers.append(vo.layer_norm(t, p["norm.weight"], p["norm.bias"]))
    return attn, layers


def _lib():
    from gipvit import _lib as L
    return L


@pytest.mark.parametrize("name,nmax", [("gv_attention_probs", 288), ("gv_attention_probs_f32", 260)])
def test_attention_probs_abi_errors(name, nmax):
    L = _lib()
    fn = getattr(L.lib, name)
    ok = dict(qkv=4096, lse=8192, p=16384, n_img=2, N=17, H=3, scale=0.125, q_rows=17)      # never dereferenced: rejected first

    def rc(**kw):
        return fn(ctypes.byref(L.gv_attention_probs_args(**dict(ok, **kw))), None)
    for k in ("qkv", "lse", "p"):
        assert rc(**{k: None}) == -3
        assert "null" in L.lib.gv_last_error().decode()
    assert rc(N=nmax + 1, q_rows=1) == -1 and str(nmax) in L.lib.gv_last_error().decode()
    assert rc(N=0, q_rows=1) == -1
    assert rc(H=0) == -1
    assert rc(q_rows=0) == -1 and "q_rows" in L.lib.gv_last_error().decode()
    assert rc(q_rows=18) == -1 and "q_rows" in L.lib.gv_last_error().decode()
    assert rc(qkv=4096 + 4) == -2 and "aligned" in L.lib.gv_last_error().decode()


def test_reference_matches_hf_vitmodel_attentions_and_hidden_states():
    from transformers import ViTConfig, ViTModel
    arch, img = "vit_tiny", 64
    a = vo.ARCHS[arch]
    D, depth = a["embed_dim"], a["depth"]
    cfg = ViTConfig(hidden_size=D, num_hidden_layers=depth, num_attention_heads=a["num_heads"], intermediate_size=4 * D, image_size=img,
                    patch_size=16, layer_norm_eps=1e-6, qkv_bias=True, hidden_act="gelu", hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, attn_implementation="eager")
    hf = ViTModel(cfg, add_pooling_layer=False).eval()
    p = vo.init_vit(arch, img, 0, seed=0)
    sd = {"embeddings.cls_token": p["cls_token"], "embeddings.position_embeddings": p["pos_embed"],
          "embeddings.patch_embeddings.projection.weight": p["patch_embed.proj.weight"],
          "embeddings.patch_embeddings.projection.bias": p["patch_embed.proj.bias"],
          "layernorm.weight": p["norm.weight"], "layernorm.bias": p["norm.bias"]}
    for i in range(depth):             # key names of transformers 5.x ViTModel (as tests/test_oracle.py)
        b, h = f"blocks.{i}.", f"layers.{i}."
        qw, qb = p[b + "attn.qkv.weight"], p[b + "attn.qkv.bias"]
        for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
            sd[h + f"attention.{nm}.weight"] = qw[j * D:(j + 1) * D]
            sd[h + f"attention.{nm}.bias"] = qb[j * D:(j + 1) * D]
        sd[h + "attention.o_proj.weight"] = p[b + "attn.proj.weight"]; sd[h + "attention.o_proj.bias"] = p[b + "attn.proj.bias"]
        sd[h + "layernorm_before.weight"] = p[b + "norm1.weight"]; sd[h + "layernorm_before.bias"] = p[b + "norm1.bias"]
        sd[h + "layernorm_after.weight"] = p[b + "norm2.weight"]; sd[h + "layernorm_after.bias"] = p[b + "norm2.bias"]
        sd[h + "mlp.fc1.weight"] = p[b + "mlp.fc1.weight"]; sd[h + "mlp.fc1.bias"] = p[b + "mlp.fc1.bias"]
        sd[h + "mlp.fc2.weight"] = p[b + "mlp.fc2.weight"]; sd[h + "mlp.fc2.bias"] = p[b + "mlp.fc2.bias"]
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not [m for m in missing if "pooler" not in m] and not unexpected, (missing, unexpected)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        out = hf(pixel_values=x, output_attentions=True, output_hidden_states=True)
        attn, layers = reference_attention_and_layers(p, x, arch)
        assert out.attentions[-1].shape == attn.shape == (2, 3, 17, 17)
        assert float((attn - out.attentions[-1]).abs().max()) <= 1e-5
        assert torch.allclose(attn.sum(-1), torch.ones(2, 3, 17), atol=1e-6)
        for k in (1, 4, 12):
            got = layers[depth - k]
            ref = hf.layernorm(out.hidden_states[-k])
            assert float((got - ref).abs().max()) <= 1e-5, (k, float((got - ref).abs().max()))
