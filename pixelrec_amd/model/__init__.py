from .basemodel import BaseModel  # noqa: F401
from .sasrec import SASRec  # noqa: F401
from .bert4rec import BERT4Rec  # noqa: F401
from .mosasrec import MOSASRec  # noqa: F401
from .fsasrec import FSASRec  # noqa: F401
from .gru4rec import GRU4Rec  # noqa: F401
from .nextitnet import NextItNet  # noqa: F401
from .mogru4rec import MOGRU4Rec  # noqa: F401
from .monextitnet import MONextItNet  # noqa: F401
from .lightgcn import LightGCN  # noqa: F401
from .srgnn import SRGNN  # noqa: F401
from .lightsans import LightSANs  # noqa: F401
from .mf import MF  # noqa: F401
from .vbpr import VBPR  # noqa: F401
from .acf import ACF  # noqa: F401
from .visrank import VISRANK  # noqa: F401
from .curatornet import CuratorNet  # noqa: F401
from .sharded import ShardedDataParallel, ShardedSASRec  # noqa: F401
