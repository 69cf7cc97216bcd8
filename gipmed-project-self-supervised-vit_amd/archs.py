"""The encoder table and the model names that select from it: plain data, importable without the HIP library (the driver checks
flags against a model's depth and width before anything is loaded)."""
from __future__ import annotations

ARCHS = {   # vit.pyc@L275-293
    "vit_tiny": dict(embed_dim=192, depth=12, num_heads=3),
    "vit_small": dict(embed_dim=384, depth=12, num_heads=6),
    "vit_base": dict(embed_dim=768, depth=12, num_heads=12),
}

# timm names used by the reference -> (arch, default img size after the documented cfg patch)
MODEL_REGISTRY = {
    "vit_tiny_patch16_224": "vit_tiny", "vit_small_patch16_224": "vit_small", "vit_base_patch16_224": "vit_base",
    "vit_small_patch16_224_dino": "vit_small", "vit_base_patch16_224_dino": "vit_base",
    "vit_tiny": "vit_tiny", "vit_small": "vit_small", "vit_base": "vit_base",
}


def resolve_arch(name: str) -> str:
    if name not in MODEL_REGISTRY:
        raise ValueError(f"unknown model '{name}'; this build covers {sorted(MODEL_REGISTRY)}")
    return MODEL_REGISTRY[name]
