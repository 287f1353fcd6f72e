"""sonic_amd -- MI355X-native Sonic prover hot path (drop-in for sdiehl/sonic's prove path).

Python host-side mirror of the reference's Haskell modules over the C ABI of
``sonic_amd/csrc/libsonic_hip.so`` (``include/sonic_hip.h``):

    Sonic.SRS               -> sonic_amd.srs          (SRS, SRS.new)
    Sonic.CommitmentScheme  -> sonic_amd.commitment   (commit_poly, open_poly, pc_v)
    Sonic.Protocol          -> sonic_amd.protocol     (prove, verify, Proof, RndOracle, Prover; Verifier / verify_batch: K proofs, one pairing product)
    Sonic.Signature         -> sonic_amd.protocol     (HscProof, hsc_prove, hsc_verify; hscProve also runs inside prove)

All compute happens in hand-written HIP kernels on the GPU; this package is ctypes plumbing.
There is no CPU fallback: without the built extension imports fail, without a GPU calls raise.
"""
import os as _os

# prove() drives the t(X,y) product and up to six MSM groups on their own HIP streams; the ROCm runtime multiplexes streams
# onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share one run behind each other.  Read when the HIP
# runtime initialises, so this only takes effect if the package is imported before the process first touches the GPU.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from ._lib import SonicError, LIB_PATH  # noqa: F401,E402
from .encoding import R_MODULUS, Q_MODULUS, fr_to_bytes, fr_from_bytes, g1_to_bytes, g1_from_bytes  # noqa: F401,E402
from .srs import SRS, srs_verify_update  # noqa: F401,E402
from .commitment import commit_poly, open_poly, pc_v, msm_g1, MsmLane  # noqa: F401,E402
from .protocol import hsc_prove_poly, hsc_verify_poly  # noqa: F401,E402
from .protocol import prove_fs, verify_fs, fs_challenges, fs_circuit_digest, fs_srs_id  # noqa: F401,E402
from .protocol import proof_from_shares, share_plan, from_x, from_y, biv_add  # noqa: F401,E402
from .protocol import prove_shared, prove_batch, prove_many, device_count  # noqa: F401,E402
from .commitment import msm_g1_srs_multi  # noqa: F401,E402
from .commitment import msm_g2, msm_g2_srs  # noqa: F401,E402
from .protocol import prove, verify, hsc_prove, hsc_verify, Proof, HscProof, RndOracle, Prover, ProverPipeline, ArithCircuit, SparseCircuit, Assignment, GateWeights  # noqa: F401,E402
from .protocol import Verifier, verify_batch  # noqa: F401,E402
from .protocol import fs_circuit_midstate, fs_circuit_digest_resume  # noqa: F401,E402
from .protocol import prove_batch_fs  # noqa: F401,E402
from .protocol import WitnessBatch  # noqa: F401,E402
from .protocol import CoreProof, prove_core_batch, prove_core_batch_fs, verify_core, verify_core_fs, fs_core_challenges  # noqa: F401,E402
from .protocol import aggregate_core, fs_weights_digest, fs_aggregate_challenges  # noqa: F401,E402
from .protocol import fs_weights_digest_v2, fs_circuit_digest_v2  # noqa: F401,E402
from .compressed import g1_compress, g1_decompress, g2_compress, g2_decompress, proof_compress, proof_decompress  # noqa: F401,E402
from .compressed import g1_subgroup_check, g2_subgroup_check  # noqa: F401,E402
from ._pairing import pairing_check, pairing  # noqa: F401,E402
from .r1cs import R1CS  # noqa: F401,E402
from . import r1cs_io  # noqa: F401,E402

__all__ = ["fs_weights_digest_v2", "fs_circuit_digest_v2", "R1CS", "r1cs_io", "pairing_check", "pairing", "g1_subgroup_check", "g2_subgroup_check", "msm_g2", "msm_g2_srs", "aggregate_core", "fs_weights_digest", "fs_aggregate_challenges", "CoreProof", "prove_core_batch", "prove_core_batch_fs", "verify_core", "verify_core_fs", "fs_core_challenges", "WitnessBatch", "Verifier", "verify_batch", "prove_batch_fs", "fs_circuit_midstate", "fs_circuit_digest_resume", "g1_compress", "g1_decompress", "g2_compress", "g2_decompress", "proof_compress", "proof_decompress", "SRS", "srs_verify_update", "commit_poly", "open_poly", "pc_v", "msm_g1", "MsmLane", "prove", "verify", "prove_fs", "verify_fs", "fs_challenges", "fs_circuit_digest", "hsc_prove", "hsc_verify", "hsc_prove_poly", "hsc_verify_poly", "Proof", "HscProof", "RndOracle", "Prover", "ProverPipeline",
           "ArithCircuit", "SparseCircuit", "Assignment", "GateWeights", "SonicError"]
