from .model import Model, GPModel
from .gpr import GPR
from .svgp import SVGP
from .sgpr import SGPR, GPRFITC
from .gplvm import GPLVM, BayesianGPLVM, PCA_reduce
from .kgpr import KGPR
from .gpmc import GPMC
from .sgpmc import SGPMC
