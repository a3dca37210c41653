from .masking import draw_keep, restore_from_keep, shuffle_tables
from .model import MAEViT
