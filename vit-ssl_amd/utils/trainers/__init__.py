from .base_trainer import BaseTrainer
from .dino_trainer import DINOTrainer
from .mae_trainer import MAETrainer
from .simmim_trainer import SimMIMTrainer
from .supervised_trainer import SupervisedTrainer
