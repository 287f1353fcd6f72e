-- | Sonic.HIP -- the reference's public surface (Sonic.SRS, Sonic.CommitmentScheme, Sonic.Protocol,
-- Sonic.Signature) over libsonic_hip.so, the MI355X prover path of this repository.
--
-- Every exported name has the type it has in sdiehl/sonic, except that `SRS` is an opaque handle to
-- device memory (its vectors are fetched on demand: `gNegativeX` .. `hPositiveAlphaX`, `srsPairing`)
-- instead of a record of lazily built vectors:
--
--   new          :: Int -> Fr -> Fr -> SRS                                       src/Sonic/SRS.hs:27-43
--   commitPoly   :: SRS -> Int -> VLaurent Fr -> G1 BLS12381                      src/Sonic/CommitmentScheme.hs:20-33
--   openPoly     :: SRS -> Fr -> VLaurent Fr -> (Fr, G1 BLS12381)                 src/Sonic/CommitmentScheme.hs:36-48
--   pcV          :: SRS -> Int -> G1 BLS12381 -> Fr -> (Fr, G1 BLS12381) -> Bool  src/Sonic/CommitmentScheme.hs:51-68
--   prove        :: MonadRandom m => SRS -> Assignment Fr -> ArithCircuit Fr -> m (Proof, RndOracle)
--                                                                                src/Sonic/Protocol.hs:47-109
--   verify       :: SRS -> ArithCircuit Fr -> Proof -> Fr -> Fr -> [(Fr, Fr)] -> Bool
--                                                                                src/Sonic/Protocol.hs:111-130
--   hscProve     :: MonadRandom m => SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof
--                                                                                src/Sonic/Signature.hs:32-72
--   hscVerify    :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool        src/Sonic/Signature.hs:74-90
--
-- plus what the reference has no counterpart for: a resident prover handle (`Prover`, `newProver`,
-- `prepare`, `proveWith`, `submit` / `collect`), one proof over several GPUs (`proveShared`), a list of
-- proofs over several GPUs (`proveBatch`), SRS persistence (`saveSRS`, `loadSRS`) and replication.
--
-- The prover's `rnd` draws stay in Haskell, in the reference's order (Protocol.hs:58,66,76,84-85;
-- Signature.hs:48,60); they cross the boundary as the explicit 8 + 2Q-element transcript, so
-- `RndOracle` is what it was.  Encodings: include/sonic_hip.h (Fr 32 bytes little-endian, G1 96 bytes
-- x || y little-endian, the point at infinity all zero, G2 192 bytes, GT 576 bytes).
--
-- Two one-token changes in the reference make the record constructors reachable from here:
--   src/Sonic/Protocol.hs:7    ( Proof      ->    ( Proof(..)
-- (HscProof(..) and RndOracle(..) are exported already).
--
-- NOT COMPILED in this repository: the build image has no ghc / cabal / stack.  tests/test_hs_shim.py
-- checks every `foreign import` below against include/sonic_hip.h (symbol exists, arity, and the kind
-- of every argument and of the result: pointer / Int64 / CInt / CSize), and tests/host/abi_harness.c
-- drives the same entry points from C99 with the calling convention `ccall` uses.
-- Dependency API used ([dep, unverified], as in SURVEY.md section 8c): galois-field 1.0.1 `fromP`, `toE`,
-- `fromE`, `toU'`; elliptic-curve 0.3.0 `Point(A, O)` of Data.Curve.Weierstrass; pairing 1.0.0 type names.
{-# LANGUAGE ForeignFunctionInterface #-}
{-# LANGUAGE RecordWildCards          #-}
{-# LANGUAGE EmptyDataDecls           #-}
module Sonic.HIP
  ( -- * Sonic.SRS
    SRS, new, newOn, replicate', srsD, srsDevice
  , gNegativeX, gPositiveX, gNegativeAlphaX, gPositiveAlphaX
  , hNegativeX, hPositiveX, hNegativeAlphaX, hPositiveAlphaX, srsPairing
  , saveSRS, loadSRS, srsForCircuit, loadSrsForCircuit
  , checkSrs, updateSrs, verifySrsUpdate, msmG2, msmG2Srs
  , g1SubgroupCheck, g2SubgroupCheck, pairingCheck
    -- * Sonic.CommitmentScheme
  , commitPoly, openPoly, pcV
    -- * Sonic.Protocol
  , prove, proveWithTranscript, verify, decodeProof, encodeProof, proofToCompressed, proofFromCompressed
  , proveWithTranscriptDense, verifyDense, fsCircuitDigest, verifyFs
    -- * Sonic.Signature
  , hscProve, hscVerify, decodeHscProof, encodeHscProof
    -- * resident handles, many GPUs
  , Prover, newProver, newProverDense, prepare, setAssignment, proveWith, submit, collect
  , proveShared, proveBatch, deviceCount
    -- * one circuit, many statements
  , setConstants, evalConstraints, proveBatchStatements, fsCircuitMidstate, fsCircuitDigestResume
  , Verifier, newVerifier, verifyBatchStatements, verifyFsBatchStatements
    -- * Fiat-Shamir proofs in flight
  , witnessDigest, submitFs, collectFs, proveBatchFs
    -- * witness sources
  , WitnessSrc(..), setWitnessI64, proveBatchI64
    -- * core proofs
  , CoreProof(..), coreOf, decodeCoreProof, encodeCoreProof, proveCore, submitCore, collectCore, proveCoreFs, verifyCore, verifyCoreBatch
    -- * Helped verification: one aggregate signature for K core proofs
  , aggregateCore, fsWeightsDigest, verifyCoreBatchHelped
    -- * R1CS front end
  , R1CS(..), R1csMatrix(..), newR1cs, r1csCircuit, r1csAssignI64
    -- * circuits with Q ~ n: weights digest v2, circuit digest v2
  , fsWeightsDigestV2, fsCircuitDigestV2, proverWeightsDigestV2, verifierWeightsDigestV2, newVerifierDigest, verifierDigestKind
  , proverDeviceBytes
  , proverHostBytes
  ) where

import Protolude hiding (check)
import qualified Data.ByteString          as BS
import qualified Data.ByteString.Internal as BSI
import qualified Data.Vector              as V
import qualified GHC.Exts
import Control.Monad.Random (MonadRandom)
import Data.Curve.Weierstrass (Point(A, O))
import Data.Field.Galois (fromE, fromP, rnd, toE, toU')
import Data.Pairing.BLS12381 (BLS12381, Fq, Fq12, Fr, G1, G2, GT)
import Data.Poly.Sparse.Laurent (VLaurent)
import Bulletproofs.ArithmeticCircuit (ArithCircuit(..), Assignment(..), GateWeights(..))
import Foreign (FunPtr, ForeignPtr, Ptr, Storable(..), alloca, allocaArray, allocaBytes, castPtr, newForeignPtr, nullPtr,
                peekElemOff, pokeArray, with, withArray, withArrayLen, withForeignPtr)
import Foreign.C.String (CString, peekCString, withCString)
import Foreign.C.Types (CChar, CInt(..), CSize(..))
import System.IO.Unsafe (unsafePerformIO)

import Sonic.Protocol (Proof(..), RndOracle(..))
import Sonic.Signature (HscProof(..))
import Sonic.Utils (BiVLaurent)

-- ---------------------------------------------------------------------------------------------------------------------
-- the C ABI (include/sonic_hip.h); `safe`: the call may block for milliseconds and must not stop the RTS
-- ---------------------------------------------------------------------------------------------------------------------
data SrsHandle
data ProverHandle

foreign import ccall unsafe "sonic_abi_version"       c_abi_version      :: IO CInt
foreign import ccall safe   "sonic_init"              c_init             :: CInt -> IO CInt
foreign import ccall safe   "sonic_device_count"      c_device_count     :: Ptr CInt -> IO CInt
foreign import ccall unsafe "sonic_last_error"        c_last_error       :: Ptr CChar -> CSize -> IO CInt

foreign import ccall safe   "sonic_srs_new"           c_srs_new          :: Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr (Ptr SrsHandle) -> IO CInt
foreign import ccall safe   "sonic_srs_new_on"        c_srs_new_on       :: CInt -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr (Ptr SrsHandle) -> IO CInt
foreign import ccall safe   "sonic_srs_replicate"     c_srs_replicate    :: Ptr SrsHandle -> CInt -> Ptr (Ptr SrsHandle) -> IO CInt
foreign import ccall safe   "&sonic_srs_free"         p_srs_free         :: FunPtr (Ptr SrsHandle -> IO ())
foreign import ccall unsafe "sonic_srs_d"             c_srs_d            :: Ptr SrsHandle -> IO Int64
foreign import ccall unsafe "sonic_srs_device"        c_srs_device       :: Ptr SrsHandle -> IO CInt
foreign import ccall safe   "sonic_srs_get_points"    c_srs_get_points   :: Ptr SrsHandle -> CInt -> Int64 -> Int64 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_srs_get_g2_points" c_srs_get_g2       :: Ptr SrsHandle -> CInt -> Int64 -> Int64 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_srs_pairing"       c_srs_pairing      :: Ptr SrsHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_srs_save"          c_srs_save         :: Ptr SrsHandle -> CString -> CInt -> IO CInt
foreign import ccall safe   "sonic_srs_load"          c_srs_load         :: CString -> Ptr (Ptr SrsHandle) -> IO CInt
foreign import ccall safe   "sonic_srs_for_circuit"   c_srs_for_circuit  :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr (Ptr SrsHandle) -> IO CInt
foreign import ccall safe   "sonic_srs_load_for_circuit" c_srs_load_for_circuit :: CString -> Int64 -> Int64 -> Ptr (Ptr SrsHandle) -> IO CInt
-- the updatable half (ABI 7): structure check, contribution, verification of a contribution
foreign import ccall safe   "sonic_srs_check"         c_srs_check        :: Ptr SrsHandle -> Ptr Word8 -> Ptr CInt -> IO CInt
foreign import ccall safe   "sonic_srs_update"        c_srs_update       :: Ptr SrsHandle -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr (Ptr SrsHandle) -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_srs_verify_update" c_srs_verify_update :: Ptr SrsHandle -> Ptr SrsHandle -> Ptr Word8 -> CInt -> Ptr CInt -> IO CInt

foreign import ccall safe   "sonic_msm_g2"            c_msm_g2           :: Ptr Word8 -> Ptr Word8 -> Int64 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_msm_g2_srs"        c_msm_g2_srs       :: Ptr SrsHandle -> CInt -> Int64 -> Ptr Word8 -> Int64 -> Ptr Word8 -> IO CInt
-- subgroup membership on its own (ABI 7); method 0: the endomorphism test of the loaders, 1: r P = O by double-and-add
foreign import ccall safe   "sonic_g1_subgroup_check" c_g1_subgroup_check :: Ptr Word8 -> Int64 -> CInt -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_g2_subgroup_check" c_g2_subgroup_check :: Ptr Word8 -> Int64 -> CInt -> Ptr Word8 -> IO CInt
-- products of pairings checked in groups (ABI 7); where 0: the library's rule, 1: host threads, 2: the GPU
foreign import ccall safe   "sonic_pairing_check"     c_pairing_check    :: Ptr Word8 -> Ptr Word8 -> Int64 -> Ptr Int64 -> Int64 -> CInt -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_commit_poly"       c_commit_poly      :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_open_poly"         c_open_poly        :: Ptr SrsHandle -> Ptr Word8 -> Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_pc_v"              c_pc_v             :: Ptr SrsHandle -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt

foreign import ccall unsafe "sonic_proof_size"        c_proof_size       :: Int64 -> IO CSize
foreign import ccall safe   "sonic_prove"             c_prove            :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verify"            c_verify           :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt
-- gate weights as CSR (ABI 7): the same calls over the non-zero entries only
foreign import ccall safe   "sonic_prove_csr"         c_prove_csr        :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verify_csr"        c_verify_csr       :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt
foreign import ccall safe   "sonic_fs_circuit_digest_csr" c_fs_digest_csr :: Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verify_fs_csr"     c_verify_fs_csr    :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt

-- compressed encodings (ABI 7, additions): one proof's re-encoding on the host, no device needed
foreign import ccall safe   "sonic_proof_size_compressed" c_proof_size_z :: Int64 -> IO CSize
foreign import ccall safe   "sonic_proof_compress"    c_proof_compress   :: Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_proof_decompress"  c_proof_decompress :: Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt

foreign import ccall unsafe "sonic_hsc_proof_size"    c_hsc_proof_size   :: Int64 -> IO CSize
foreign import ccall safe   "sonic_hsc_prove_poly"    c_hsc_prove_poly   :: Ptr SrsHandle -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_hsc_verify_poly"   c_hsc_verify_poly  :: Ptr SrsHandle -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt

foreign import ccall safe   "sonic_prover_new"            c_prover_new     :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr (Ptr ProverHandle) -> IO CInt
foreign import ccall safe   "sonic_prover_new_csr"        c_prover_new_csr :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr (Ptr ProverHandle) -> IO CInt
foreign import ccall safe   "&sonic_prover_free"          p_prover_free    :: FunPtr (Ptr ProverHandle -> IO ())
foreign import ccall safe   "sonic_prover_prepare"        c_prover_prepare :: Ptr ProverHandle -> IO CInt
foreign import ccall safe   "sonic_prover_set_assignment" c_prover_set     :: Ptr ProverHandle -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_prove"          c_prover_prove   :: Ptr ProverHandle -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_submit"         c_prover_submit  :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_collect"        c_prover_collect :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prove_shared"          c_prove_shared   :: Ptr (Ptr ProverHandle) -> CInt -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prove_batch"           c_prove_batch    :: Ptr (Ptr ProverHandle) -> CInt -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt

-- one circuit, many statements (ABI 7, additions): per-proof constants on a resident circuit, prover and batched verifier
data VerifierHandle
foreign import ccall safe   "sonic_prover_eval_constraints" c_eval_constraints :: Ptr ProverHandle -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Int64 -> IO CInt
foreign import ccall safe   "sonic_prover_set_constants"  c_set_constants  :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prove_batch_statements" c_prove_batch_st :: Ptr (Ptr ProverHandle) -> CInt -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt
foreign import ccall safe   "sonic_fs_circuit_midstate_csr" c_fs_midstate_csr :: Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_fs_circuit_digest_resume" c_fs_resume   :: Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_witness_digest_v2" c_witness_digest :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_submit_fs"      c_prover_submit_fs :: Ptr ProverHandle -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_collect_fs"     c_prover_collect_fs :: Ptr ProverHandle -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prove_batch_fs"        c_prove_batch_fs :: Ptr (Ptr ProverHandle) -> CInt -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt
-- witness sources (ABI 7, additions): where an assignment comes from, as one description (sonic_witness_src_t)
foreign import ccall safe   "sonic_prover_set_witness"    c_prover_set_witness :: Ptr ProverHandle -> Ptr WitnessSrc -> IO CInt
foreign import ccall safe   "sonic_prove_batch_src"       c_prove_batch_src :: Ptr (Ptr ProverHandle) -> CInt -> Int64 -> Ptr WitnessSrc -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt
foreign import ccall safe   "sonic_verifier_new_csr"      c_verifier_new_csr :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr (Ptr VerifierHandle) -> IO CInt
foreign import ccall safe   "&sonic_verifier_free"        p_verifier_free  :: FunPtr (Ptr VerifierHandle -> IO ())
foreign import ccall safe   "sonic_verifier_verify_batch_cs" c_verify_batch_cs :: Ptr VerifierHandle -> Int64 -> Ptr Word8 -> CInt -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_prove_core"     c_prover_prove_core :: Ptr ProverHandle -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_submit_core"    c_prover_submit_core :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_collect_core"   c_prover_collect_core :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_prove_core_fs"  c_prover_prove_core_fs :: Ptr ProverHandle -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_fs_weights_digest"     c_fs_weights_digest :: Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_fs_weights_digest_v2_csr" c_fs_weights_digest_v2 :: Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_fs_circuit_digest_v2"  c_fs_circuit_digest_v2 :: Ptr Word8 -> Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_prover_weights_digest_v2" c_prover_weights_digest_v2 :: Ptr ProverHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verifier_weights_digest_v2" c_verifier_weights_digest_v2 :: Ptr VerifierHandle -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verifier_new_digest"   c_verifier_new_digest :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> CInt -> Ptr (Ptr VerifierHandle) -> IO CInt
foreign import ccall safe   "sonic_verifier_digest_kind"  c_verifier_digest_kind :: Ptr VerifierHandle -> IO CInt
foreign import ccall safe   "sonic_prover_device_bytes"   c_prover_device_bytes :: Ptr ProverHandle -> Ptr Int64 -> IO CInt
foreign import ccall safe   "sonic_prover_host_bytes"   c_prover_host_bytes :: Ptr ProverHandle -> Ptr Int64 -> IO CInt
foreign import ccall safe   "sonic_prover_aggregate_core" c_prover_aggregate_core :: Ptr ProverHandle -> Ptr Word8 -> Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verifier_verify_core_batch_helped" c_verify_core_batch_helped :: Ptr VerifierHandle -> Int64 -> Ptr Word8 -> CInt -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verify_core_csr"       c_verify_core_csr :: Ptr SrsHandle -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> IO CInt
foreign import ccall safe   "sonic_verifier_verify_core_batch" c_verify_core_batch :: Ptr VerifierHandle -> Int64 -> Ptr Word8 -> CInt -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_verifier_verify_fs_batch_cs" c_verify_fs_batch_cs :: Ptr VerifierHandle -> Int64 -> Ptr Word8 -> CInt -> Ptr Word8 -> Ptr Word8 -> Ptr CInt -> Ptr Word8 -> IO CInt
-- R1CS front end (ABI 7, additions): A, B, C resident on one GPU, compiled to a Sonic CSR, witnesses turned into assignments
foreign import ccall safe   "sonic_r1cs_new"              c_r1cs_new       :: Int64 -> Int64 -> Int64 -> Ptr R1csMatrix -> Ptr R1csMatrix -> Ptr R1csMatrix -> Ptr (Ptr R1csHandle) -> IO CInt
foreign import ccall safe   "&sonic_r1cs_free"            p_r1cs_free      :: FunPtr (Ptr R1csHandle -> IO ())
foreign import ccall safe   "sonic_r1cs_shape"            c_r1cs_shape     :: Ptr R1csHandle -> Ptr Int64 -> IO CInt
foreign import ccall safe   "sonic_r1cs_circuit"          c_r1cs_circuit   :: Ptr R1csHandle -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe   "sonic_r1cs_assign"           c_r1cs_assign    :: Ptr R1csHandle -> Int64 -> Ptr () -> CInt -> CInt -> Int64 -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Int64 -> Ptr Word8 -> Ptr Int64 -> IO CInt

-- ---------------------------------------------------------------------------------------------------------------------
-- status codes -> the reference's failure behaviour (it panics: Protocol.hs:55, CommitmentScheme.hs:70-73, :44)
-- ---------------------------------------------------------------------------------------------------------------------
lastError :: IO Text
lastError = allocaBytes 512 $ \buf -> do
  _ <- c_last_error buf 512
  toS <$> peekCString buf

check :: CInt -> IO ()
check 0 = pure ()
check 1 = lastError >>= panic                                     -- "Parameter d is not large enough: .."   Protocol.hs:55
check 2 = lastError >>= \m -> panic (m <> " (is not long enough)")  -- `index`                              CommitmentScheme.hs:70-73
check 4 = lastError >>= \m -> panic ("fromJust: " <> m)             -- inexact division                     CommitmentScheme.hs:44
check c = lastError >>= \m -> panic ("libsonic_hip status " <> show c <> ": " <> m)

abiExpected :: CInt
abiExpected = 7

-- every entry into the library goes through here once: the header this module was written against
libraryReady :: ()
libraryReady = unsafePerformIO $ do
  v <- c_abi_version
  when (v /= abiExpected) $ panic ("libsonic_hip: ABI version " <> show v <> ", this binding expects " <> show abiExpected)
  check =<< c_init (-1)
{-# NOINLINE libraryReady #-}

-- ---------------------------------------------------------------------------------------------------------------------
-- marshalling: little-endian integers, affine points, towers
-- ---------------------------------------------------------------------------------------------------------------------
leBytes :: Int -> Integer -> ByteString
leBytes len v = fst (BS.unfoldrN len (\x -> Just (fromIntegral (x `mod` 256), x `div` 256)) v)

leInteger :: ByteString -> Integer
leInteger = BS.foldr' (\b acc -> acc * 256 + fromIntegral b) 0

frToBytes :: Fr -> ByteString
frToBytes = leBytes 32 . fromP

frFromBytes :: ByteString -> Fr
frFromBytes = fromInteger . leInteger

fqToBytes :: Fq -> ByteString
fqToBytes = leBytes 48 . fromP

fqFromBytes :: ByteString -> Fq
fqFromBytes = fromInteger . leInteger

-- | `A x y` <-> x || y, `O` (mempty) <-> 96 zero bytes ((0, 0) is not on y^2 = x^3 + 4)
g1ToBytes :: G1 BLS12381 -> ByteString
g1ToBytes O       = BS.replicate 96 0
g1ToBytes (A x y) = fqToBytes x <> fqToBytes y

g1FromBytes :: ByteString -> G1 BLS12381
g1FromBytes b
  | BS.all (== 0) b = O
  | otherwise       = A (fqFromBytes (BS.take 48 b)) (fqFromBytes (BS.take 48 (BS.drop 48 b)))

-- | G2: x.c0 || x.c1 || y.c0 || y.c1, x = c0 + c1 u (Fq2 = Fq[u]/(u^2 + 1)); infinity = 192 zero bytes
g2FromBytes :: ByteString -> G2 BLS12381
g2FromBytes b
  | BS.all (== 0) b = O
  | otherwise       = A (toE [c 0, c 1]) (toE [c 2, c 3])
  where c i = fqFromBytes (BS.take 48 (BS.drop (48 * i) b))

g2ToBytes :: G2 BLS12381 -> ByteString
g2ToBytes O       = BS.replicate 192 0
g2ToBytes (A x y) = BS.concat (map fqToBytes (coeffs x ++ coeffs y))
  where coeffs e = take 2 (fromE e ++ repeat 0)             -- (a coefficient list may stop at the last non-zero one)

-- | GT: the Fq12 element as its twelve Fq coefficients in tower order, c[i][j][k] at 48 (6 i + 2 j + k)
--   (Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (1 + u)), Fq2 = Fq[u]/(u^2 + 1))
fq12FromBytes :: ByteString -> Fq12
fq12FromBytes b = toE [ toE [ toE [c i j 0, c i j 1] | j <- [0, 1, 2] ] | i <- [0, 1] ]
  where c i j k = fqFromBytes (BS.take 48 (BS.drop (48 * (6 * i + 2 * j + k)) b))

fq12ToBytes :: Fq12 -> ByteString
fq12ToBytes x = BS.concat [ fqToBytes c | h <- fromE x, f2 <- fromE h, c <- fromE f2 ]

withBytes :: ByteString -> (Ptr Word8 -> IO a) -> IO a
withBytes b f = BS.useAsCString b (f . castPtr)             -- (copies; never a null pointer, also for an empty list)

withFr :: Fr -> (Ptr Word8 -> IO a) -> IO a
withFr = withBytes . frToBytes

withFrs :: [Fr] -> (Ptr Word8 -> IO a) -> IO a
withFrs = withBytes . BS.concat . map frToBytes

withG1 :: G1 BLS12381 -> (Ptr Word8 -> IO a) -> IO a
withG1 = withBytes . g1ToBytes

-- | the `(Int, Fr)` list that `GHC.Exts.toList` yields for a VLaurent (CommitmentScheme.hs:33,48)
withTerms :: [(Int, Fr)] -> (Int64 -> Ptr Int64 -> Ptr Word8 -> IO a) -> IO a
withTerms ts f =
  withArrayLen (map (fromIntegral . fst) ts) $ \n es ->
    withFrs (map snd ts) $ \cs -> f (fromIntegral n) es cs

-- | BiVLaurent Fr = VLaurent (VLaurent Fr): X outside, Y inside (Utils.hs:15-21) -> three parallel arrays
withBiTerms :: BiVLaurent Fr -> (Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> IO a) -> IO a
withBiTerms sXY f =
  let ts = [ (i, j, c) | (i, inner) <- GHC.Exts.toList sXY, (j, c) <- GHC.Exts.toList inner ]
  in withArrayLen [ fromIntegral i | (i, _, _) <- ts ] $ \n xs ->
       withArrayLen [ fromIntegral j | (_, j, _) <- ts ] $ \_ ys ->
         withFrs [ c | (_, _, c) <- ts ] $ \cs -> f (fromIntegral n) xs ys cs

packed :: Ptr Word8 -> Int -> IO ByteString
packed p len = BS.packCStringLen (castPtr p, len)

chunks :: Int -> ByteString -> [ByteString]
chunks k b | BS.null b = []
           | otherwise = BS.take k b : chunks k (BS.drop k b)

-- ---------------------------------------------------------------------------------------------------------------------
-- Sonic.SRS
-- ---------------------------------------------------------------------------------------------------------------------
-- | the reference's record of ten fields (SRS.hs:11-22) as a handle: d and a finalizer; the vectors live in HBM
newtype SRS = SRS (ForeignPtr SrsHandle)

wrapSRS :: Ptr (Ptr SrsHandle) -> IO SRS
wrapSRS out = SRS <$> (newForeignPtr p_srs_free =<< peek out)

-- | SRS.new :: Int -> Fr -> Fr -> SRS   (src/Sonic/SRS.hs:27-43); generated on the default GPU
new :: Int -> Fr -> Fr -> SRS
new d x alpha = libraryReady `seq` unsafePerformIO (
  withFr x $ \px -> withFr alpha $ \pa -> alloca $ \out -> do
    check =<< c_srs_new (fromIntegral d) px pa out
    wrapSRS out)
{-# NOINLINE new #-}

-- | the same on a named GPU
newOn :: Int -> Int -> Fr -> Fr -> IO SRS
newOn device d x alpha = libraryReady `seq`
  withFr x $ \px -> withFr alpha $ \pa -> alloca $ \out -> do
    check =<< c_srs_new_on (fromIntegral device) (fromIntegral d) px pa out
    wrapSRS out

-- | a replica on another GPU (device-to-device copy of the bases and their window tables)
replicate' :: SRS -> Int -> IO SRS
replicate' (SRS h) device = withForeignPtr h $ \p -> alloca $ \out -> do
  check =<< c_srs_replicate p (fromIntegral device) out
  wrapSRS out

srsD :: SRS -> Int
srsD (SRS h) = unsafePerformIO (withForeignPtr h (fmap fromIntegral . c_srs_d))

srsDevice :: SRS -> Int
srsDevice (SRS h) = unsafePerformIO (withForeignPtr h (fmap fromIntegral . c_srs_device))

-- exponents e0 .. e0 + n - 1 of one basis (0: g^{x^e}, 1: g^{alpha x^e}); SRS.hs:33-39 index maps in include/sonic_hip.h
g1Range :: SRS -> CInt -> Int -> Int -> [G1 BLS12381]
g1Range (SRS h) basis e0 n = unsafePerformIO $
  withForeignPtr h $ \p -> allocaBytes (96 * max 1 n) $ \out -> do
    check =<< c_srs_get_points p basis (fromIntegral e0) (fromIntegral n) out
    map g1FromBytes . chunks 96 <$> packed out (96 * n)

g2Range :: SRS -> CInt -> Int -> Int -> [G2 BLS12381]
g2Range (SRS h) basis e0 n = unsafePerformIO $
  withForeignPtr h $ \p -> allocaBytes (192 * max 1 n) $ \out -> do
    check =<< c_srs_get_g2 p basis (fromIntegral e0) (fromIntegral n) out
    map g2FromBytes . chunks 192 <$> packed out (192 * n)

gNegativeX, gPositiveX, gNegativeAlphaX, gPositiveAlphaX :: SRS -> V.Vector (G1 BLS12381)
gNegativeX      s = V.fromList (reverse (g1Range s 0 (negate (srsD s)) (srsD s)))       -- [k] = g^{x^{-(k+1)}}
gPositiveX      s = V.fromList (g1Range s 0 0 (srsD s + 1))                             -- [k] = g^{x^k}
gNegativeAlphaX s = V.fromList (reverse (g1Range s 1 (negate (srsD s)) (srsD s)))       -- [k] = g^{alpha x^{-(k+1)}}
gPositiveAlphaX s = V.fromList (g1Range s 1 1 (srsD s))                                 -- [k] = g^{alpha x^{k+1}}: g^alpha is not shared

hNegativeX, hPositiveX, hNegativeAlphaX, hPositiveAlphaX :: SRS -> V.Vector (G2 BLS12381)
hNegativeX      s = V.fromList (reverse (g2Range s 0 (negate (srsD s)) (srsD s)))
hPositiveX      s = V.fromList (g2Range s 0 0 (srsD s + 1))
hNegativeAlphaX s = V.fromList (reverse (g2Range s 1 (negate (srsD s)) (srsD s)))
hPositiveAlphaX s = V.fromList (g2Range s 1 0 (srsD s + 1))                             -- [0] = h^alpha (SRS.hs:41)

-- | srsPairing = pairing gen (hPositiveAlphaX !! 0)    (src/Sonic/SRS.hs:21,42)
srsPairing :: SRS -> GT BLS12381
srsPairing (SRS h) = unsafePerformIO $
  withForeignPtr h $ \p -> allocaBytes 576 $ \out -> do
    check =<< c_srs_pairing p out
    toU' . fq12FromBytes <$> packed out 576

-- | persistence (nothing in the reference): withG2 = write the verifier half as well
saveSRS :: SRS -> FilePath -> Bool -> IO ()
saveSRS (SRS h) path withG2 = withForeignPtr h $ \p -> withCString path $ \cp ->
  check =<< c_srs_save p cp (if withG2 then 1 else 0)

loadSRS :: FilePath -> IO SRS
loadSRS path = libraryReady `seq` withCString path (\cp -> alloca $ \out -> do
  check =<< c_srs_load cp out
  wrapSRS out)

-- | a circuit-sized view of a universal string (include/sonic_hip.h, "circuit-sized views"): the same d, the same proofs, over copies
-- of only the exponents a circuit of n gates and q constraints touches; the string itself may be dropped afterwards
srsForCircuit :: SRS -> Int -> Int -> IO SRS
srsForCircuit (SRS h) n q = withForeignPtr h $ \p -> alloca $ \out -> do
  check =<< c_srs_for_circuit p (fromIntegral n) (fromIntegral q) out
  wrapSRS out

-- | the same view read from a file of either container: only the byte ranges of its windows are read
loadSrsForCircuit :: FilePath -> Int -> Int -> IO SRS
loadSrsForCircuit path n q = libraryReady `seq` withCString path (\cp -> alloca $ \out -> do
  check =<< c_srs_load_for_circuit cp (fromIntegral n) (fromIntegral q) out
  wrapSRS out)

-- | whether the handle's points ARE a reference string (include/sonic_hip.h, "Updatable SRS": relations R0 .. R4 under random 128-bit
-- weights drawn from the operating system).  Right (): it passes; Left mask: bit i set when Ri fails.  Run it on every string that
-- comes from outside: loading validates each point on its own and nothing else.
checkSrs :: SRS -> IO (Either Int ())
checkSrs (SRS h) = withForeignPtr h $ \p -> alloca $ \failed -> do
  check =<< c_srs_check p nullPtr failed
  m <- peek failed
  pure (if m == 0 then Right () else Left (fromIntegral m))

-- | a contribution with shares x1, alpha1 (non-zero): the string of trapdoor (x x1, alpha alpha1) as a NEW handle on the same GPU, and
-- the 448-byte proof that the contributor knew the shares.  The source is untouched.  Nonces come from the operating system.
updateSrs :: SRS -> Fr -> Fr -> IO (SRS, ByteString)
updateSrs (SRS h) x1 alpha1 = withForeignPtr h $ \p -> withFr x1 $ \px -> withFr alpha1 $ \pa ->
  alloca $ \out -> allocaBytes 448 $ \proof -> do
    check =<< c_srs_update p px pa nullPtr out proof
    (,) <$> wrapSRS out <*> packed proof 448

-- | whether the second string is the first updated by someone who knew the shares behind the proof; the new string's structure is
-- checked as well (checkSrs).  A malformed proof is False.
verifySrsUpdate :: SRS -> SRS -> ByteString -> IO Bool
verifySrsUpdate (SRS old) (SRS new') proof
  | BS.length proof /= 448 = pure False
  | otherwise = withForeignPtr old $ \po -> withForeignPtr new' $ \pn -> withBytes proof $ \pp -> alloca $ \ok -> do
      check =<< c_srs_verify_update po pn pp 1 ok
      (/= 0) <$> peek ok

-- | sum_i s_i P_i on the twist (include/sonic_hip.h, sonic_msm_g2): the points only have to be on the twist (O is the neutral element)
-- and the sum is the literal multiple, whatever subgroup they lie in
msmG2 :: [(G2 BLS12381, Fr)] -> IO (G2 BLS12381)
msmG2 terms = libraryReady `seq`
  withBytes (BS.concat (map (g2ToBytes . fst) terms)) $ \pp -> withFrs (map snd terms) $ \ps ->
    allocaBytes 192 $ \out -> do
      check =<< c_msm_g2 pp ps (fromIntegral (length terms)) out
      g2FromBytes <$> packed out 192

-- | sum_i s_i H[e0 + i] over the G2 half of the string: basis 0 is h^{x^e}, basis 1 h^{alpha x^e} (sonic_msm_g2_srs) -- a commitment in
-- G2, e.g. to check a counterparty's polynomial against the string
msmG2Srs :: SRS -> Int -> Int -> [Fr] -> IO (G2 BLS12381)
msmG2Srs (SRS h) basis e0 scalars = withForeignPtr h $ \p -> withFrs scalars $ \ps ->
  allocaBytes 192 $ \out -> do
    check =<< c_msm_g2_srs p (fromIntegral basis) (fromIntegral e0) ps (fromIntegral (length scalars)) out
    g2FromBytes <$> packed out 192

-- | whether each point lies in the order-r subgroup (include/sonic_hip.h, "Subgroup membership": phi(P) = lambda P on the GPU, one thread
-- per point; O is a member).  Values of the curve's type are canonical and on the curve, so False means: outside the subgroup.
g1SubgroupCheck :: [G1 BLS12381] -> IO [Bool]
g1SubgroupCheck pts = libraryReady `seq`
  withBytes (BS.concat (map g1ToBytes pts)) $ \pp -> allocaBytes (max 1 (length pts)) $ \fl -> do
    check =<< c_g1_subgroup_check pp (fromIntegral (length pts)) 0 fl
    map (== 0) . BS.unpack <$> packed fl (length pts)

-- | the same over the twist (psi(P) = z P): run it over the operands of msmG2 when they come from outside
g2SubgroupCheck :: [G2 BLS12381] -> IO [Bool]
g2SubgroupCheck pts = libraryReady `seq`
  withBytes (BS.concat (map g2ToBytes pts)) $ \pp -> allocaBytes (max 1 (length pts)) $ \fl -> do
    check =<< c_g2_subgroup_check pp (fromIntegral (length pts)) 0 fl
    map (== 0) . BS.unpack <$> packed fl (length pts)

-- | one verdict per group of pairs: whether the product of the group's pairings is one (include/sonic_hip.h, "Pairing": KZG openings,
-- batches of BLS signatures, the links of an SRS ceremony).  Values of the curves' types are canonical and on the curve; a point outside
-- the order-r subgroup makes its group False.  An empty group is True.
pairingCheck :: [[(G1 BLS12381, G2 BLS12381)]] -> IO [Bool]
pairingCheck groups = libraryReady `seq`
  let pairs = concat groups
      ends  = drop 1 (scanl (+) 0 (map length groups))
  in withBytes (BS.concat (map (g1ToBytes . fst) pairs)) $ \p1 -> withBytes (BS.concat (map (g2ToBytes . snd) pairs)) $ \p2 ->
       withArrayLen (map fromIntegral ends :: [Int64]) $ \ng pe -> allocaBytes (max 1 ng) $ \vd -> do
         check =<< c_pairing_check p1 p2 (fromIntegral (length pairs)) pe (fromIntegral ng) 0 vd nullPtr
         map (== 0) . BS.unpack <$> packed vd ng

-- ---------------------------------------------------------------------------------------------------------------------
-- Sonic.CommitmentScheme
-- ---------------------------------------------------------------------------------------------------------------------
-- | commitPoly :: SRS -> Int -> VLaurent Fr -> G1 BLS12381      (src/Sonic/CommitmentScheme.hs:20-33)
commitPoly :: SRS -> Int -> VLaurent Fr -> G1 BLS12381
commitPoly (SRS h) maxm fX = unsafePerformIO $
  withForeignPtr h $ \p -> withTerms (GHC.Exts.toList fX) $ \n es cs ->
    allocaBytes 96 $ \out -> do
      check =<< c_commit_poly p (fromIntegral maxm) n es cs out
      g1FromBytes <$> packed out 96

-- | openPoly :: SRS -> Fr -> VLaurent Fr -> (Fr, G1 BLS12381)   (src/Sonic/CommitmentScheme.hs:36-48)
openPoly :: SRS -> Fr -> VLaurent Fr -> (Fr, G1 BLS12381)
openPoly (SRS h) z fX = unsafePerformIO $
  withForeignPtr h $ \p -> withFr z $ \pz -> withTerms (GHC.Exts.toList fX) $ \n es cs ->
    allocaBytes 32 $ \fz -> allocaBytes 96 $ \out -> do
      check =<< c_open_poly p pz n es cs fz out
      (,) <$> (frFromBytes <$> packed fz 32) <*> (g1FromBytes <$> packed out 96)

-- | pcV :: SRS -> Int -> G1 BLS12381 -> Fr -> (Fr, G1 BLS12381) -> Bool   (src/Sonic/CommitmentScheme.hs:51-68)
pcV :: SRS -> Int -> G1 BLS12381 -> Fr -> (Fr, G1 BLS12381) -> Bool
pcV (SRS h) maxm commitment z (v, w) = unsafePerformIO $
  withForeignPtr h $ \p -> withG1 commitment $ \pc -> withFr z $ \pz -> withFr v $ \pv -> withG1 w $ \pw ->
    alloca $ \acc -> do
      check =<< c_pc_v p (fromIntegral maxm) pc pz pv pw acc
      (/= 0) <$> peek acc

-- ---------------------------------------------------------------------------------------------------------------------
-- proof bytes <-> the records (include/sonic_hip.h: record order of `Proof`, Protocol.hs:28-38, then `HscProof`,
-- Signature.hs:22-29):  R T a Wa b Wb Wt s  [S_j s_j W_j]_j  [s'_j W'_j Q_j]_j  Qv C u v
-- ---------------------------------------------------------------------------------------------------------------------
takeG :: ByteString -> (G1 BLS12381, ByteString)
takeG b = (g1FromBytes (BS.take 96 b), BS.drop 96 b)

takeF :: ByteString -> (Fr, ByteString)
takeF b = (frFromBytes (BS.take 32 b), BS.drop 32 b)

-- | the HscProof part: (2 + 4 m) G1 + (2 + 2 m) Fr
decodeHscProof :: Int -> ByteString -> HscProof
decodeHscProof m b0 =
  let goS :: Int -> ByteString -> ([(G1 BLS12381, (Fr, G1 BLS12381))], ByteString)
      goS 0 b = ([], b)
      goS k b = let (sj, b1) = takeG b; (ev, b2) = takeF b1; (wj, b3) = takeG b2
                    (rest, b4) = goS (k - 1) b3
                in ((sj, (ev, wj)) : rest, b4)
      goW :: Int -> ByteString -> ([(Fr, G1 BLS12381, G1 BLS12381)], ByteString)
      goW 0 b = ([], b)
      goW k b = let (ev, b1) = takeF b; (wj', b2) = takeG b1; (qj, b3) = takeG b2
                    (rest, b4) = goW (k - 1) b3
                in ((ev, wj', qj) : rest, b4)
      (ss, c1) = goS m b0
      (ws, c2) = goW m c1
      (qv, c3) = takeG c2
      (cc, c4) = takeG c3
      (u, c5)  = takeF c4
      (v, _)   = takeF c5
  in HscProof { hscS = ss, hscW = ws, hscQv = qv, hscC = cc, hscU = u, hscV = v }

encodeHscProof :: HscProof -> ByteString
encodeHscProof HscProof{..} = BS.concat $
  [ g1ToBytes sj <> frToBytes ev <> g1ToBytes wj | (sj, (ev, wj)) <- hscS ] ++
  [ frToBytes ev <> g1ToBytes wj' <> g1ToBytes qj | (ev, wj', qj) <- hscW ] ++
  [ g1ToBytes hscQv, g1ToBytes hscC, frToBytes hscU, frToBytes hscV ]

-- | (7 + 4Q) G1 + (5 + 2Q) Fr
decodeProof :: Int -> ByteString -> Proof
decodeProof q b0 =
  let (r, b1)  = takeG b0
      (t, b2)  = takeG b1
      (a, b3)  = takeF b2
      (wa, b4) = takeG b3
      (b, b5)  = takeF b4
      (wb, b6) = takeG b5
      (wt, b7) = takeG b6
      (s, b8)  = takeF b7
  in Proof { prR = r, prT = t, prA = a, prWa = wa, prB = b, prWb = wb, prWt = wt, prS = s
           , prHscProof = decodeHscProof q b8 }

encodeProof :: Proof -> ByteString
encodeProof Proof{..} = BS.concat
  [ g1ToBytes prR, g1ToBytes prT, frToBytes prA, g1ToBytes prWa, frToBytes prB, g1ToBytes prWb, g1ToBytes prWt, frToBytes prS
  , encodeHscProof prHscProof ]

-- | the proof in the compressed wire format of other BLS12-381 libraries (include/sonic_hip.h, "Compressed encodings"): every point as
--   its 48 bytes, the field elements untouched -- (7 + 4Q) * 48 + (5 + 2Q) * 32 bytes.  The points are validated; a proof the verifier
--   would refuse as malformed panics here like every other refused input.
proofToCompressed :: Proof -> ByteString
proofToCompressed proof = unsafePerformIO $ do
  let q = fromIntegral (length (hscS (prHscProof proof))) :: Int64
  sz <- fromIntegral <$> c_proof_size_z q
  withBytes (encodeProof proof) $ \src ->
    BSI.create sz $ \out -> check =<< c_proof_compress q src out

-- | the inverse, for a proof of Q linear constraints: malformed, off-curve and out-of-subgroup points and non-canonical field elements panic
proofFromCompressed :: Int -> ByteString -> Proof
proofFromCompressed q bytes = unsafePerformIO $ do
  want <- fromIntegral <$> c_proof_size_z (fromIntegral q)
  when (BS.length bytes /= want) $ panic ("proofFromCompressed: expected " <> show want <> " bytes, got " <> show (BS.length bytes))
  sz <- fromIntegral <$> c_proof_size (fromIntegral q)
  raw <- withBytes bytes $ \src ->
    BSI.create sz $ \out -> check =<< c_proof_decompress (fromIntegral q) src out
  pure (decodeProof q raw)

-- ---------------------------------------------------------------------------------------------------------------------
-- Sonic.Protocol
-- ---------------------------------------------------------------------------------------------------------------------
-- dense Q x n row-major weights, as include/sonic_hip.h takes them (the *Dense functions)
withCircuit :: ArithCircuit Fr -> (Int64 -> Int64 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> Ptr Word8 -> IO a) -> IO a
withCircuit ArithCircuit{..} f =
  let GateWeights{..} = weights
      q = length wL
      n = case wL of { (row : _) -> length row; [] -> 0 }
  in withFrs (concat wL) $ \pwl -> withFrs (concat wR) $ \pwr -> withFrs (concat wO) $ \pwo -> withFrs cs $ \pcs ->
       f (fromIntegral n) (fromIntegral q) pwl pwr pwo pcs

-- the same weights as ONE CSR of 3Q rows (include/sonic_hip.h, "gate weights as CSR"): wL's rows, then wR's, then wO's, each walked once
-- with its zeros dropped -- the reference's circuits are lists of mostly-zero rows (Constraints.hs:34-53), and the library's cost of
-- the circuit follows the entries instead of Q x n
withCircuitCsr :: ArithCircuit Fr -> (Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Word8 -> Ptr Word8 -> IO a) -> IO a
withCircuitCsr ArithCircuit{..} f =
  let GateWeights{..} = weights
      q = length wL
      n = case wL of { (row : _) -> length row; [] -> 0 }
      rows = [ [ (i, c) | (i, c) <- zip [0 :: Int ..] row, c /= 0 ] | row <- wL ++ wR ++ wO ]
      rowPtr = scanl (+) 0 (map length rows)
      entries = concat rows
  in withArrayLen (map fromIntegral rowPtr :: [Int64]) $ \_ prp ->
       withArrayLen (map (fromIntegral . fst) entries :: [Int64]) $ \_ pcol ->
         withFrs (map snd entries) $ \pval -> withFrs cs $ \pcs ->
           f (fromIntegral n) (fromIntegral q) prp pcol pval pcs

-- | the draws of `prove` + `hscProve` in the reference's order: c_{n+1..n+4}, y, z, y_1..y_Q, z_1..z_Q, u, v
drawTranscript :: MonadRandom m => Int -> m ([Fr], RndOracle)
drawTranscript q = do
  cns <- replicateM 4 rnd               -- Protocol.hs:58
  y   <- rnd                            -- :66
  z   <- rnd                            -- :76
  ys  <- replicateM q rnd               -- :84
  zs  <- replicateM q rnd               -- :85
  u   <- rnd                            -- Signature.hs:48
  v   <- rnd                            -- :60
  pure (cns ++ [y, z] ++ ys ++ zs ++ [u, v], RndOracle { rndOracleY = y, rndOracleZ = z, rndOracleYZs = zip ys zs })

-- | prove with the draws supplied by the caller (what makes proofs reproducible; the tests of this repository use it)
proveWithTranscript :: SRS -> Assignment Fr -> ArithCircuit Fr -> [Fr] -> Proof
proveWithTranscript (SRS h) Assignment{..} circuit transcript = unsafePerformIO $
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \_ q prp pcol pval pcs ->
    withFrs aL $ \pal -> withFrs aR $ \par -> withFrs aO $ \pao -> withFrs transcript $ \ptr -> do
      sz <- fromIntegral <$> c_proof_size q
      bytes <- BSI.create sz $ \out ->
        check =<< c_prove_csr p (fromIntegral (length aL)) q prp pcol pval pcs pal par pao ptr out
      pure (decodeProof (fromIntegral q) bytes)

-- | proveWithTranscript over the dense Q x n weight arrays (sonic_prove): the same bytes
proveWithTranscriptDense :: SRS -> Assignment Fr -> ArithCircuit Fr -> [Fr] -> Proof
proveWithTranscriptDense (SRS h) Assignment{..} circuit transcript = unsafePerformIO $
  withForeignPtr h $ \p -> withCircuit circuit $ \_ q pwl pwr pwo pcs ->
    withFrs aL $ \pal -> withFrs aR $ \par -> withFrs aO $ \pao -> withFrs transcript $ \ptr -> do
      sz <- fromIntegral <$> c_proof_size q
      bytes <- BSI.create sz $ \out ->
        check =<< c_prove p (fromIntegral (length aL)) q pwl pwr pwo pcs pal par pao ptr out
      pure (decodeProof (fromIntegral q) bytes)

-- | prove :: MonadRandom m => SRS -> Assignment Fr -> ArithCircuit Fr -> m (Proof, RndOracle)
--   (src/Sonic/Protocol.hs:47-109, with hscProve, src/Sonic/Signature.hs:38-72, inside)
prove :: MonadRandom m => SRS -> Assignment Fr -> ArithCircuit Fr -> m (Proof, RndOracle)
prove srs assignment circuit = do
  (transcript, oracle) <- drawTranscript (length (wL (weights circuit)))
  pure (proveWithTranscript srs assignment circuit transcript, oracle)

-- | verify :: SRS -> ArithCircuit Fr -> Proof -> Fr -> Fr -> [(Fr, Fr)] -> Bool   (src/Sonic/Protocol.hs:111-130)
--   host CPU inside the library (its own pairing); the reference's `verify` on the points `decodeProof` returns is equivalent
verify :: SRS -> ArithCircuit Fr -> Proof -> Fr -> Fr -> [(Fr, Fr)] -> Bool
verify (SRS h) circuit proof y z yzs = unsafePerformIO $
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \n q prp pcol pval pcs ->
    withBytes (encodeProof proof) $ \ppf -> withFr y $ \py -> withFr z $ \pz ->
      withFrs (concat [ [yj, zj] | (yj, zj) <- yzs ]) $ \pyz -> alloca $ \acc -> do
        check =<< c_verify_csr p n q prp pcol pval pcs ppf py pz pyz acc
        (/= 0) <$> peek acc

-- | verify over the dense Q x n weight arrays (sonic_verify): the same answer
verifyDense :: SRS -> ArithCircuit Fr -> Proof -> Fr -> Fr -> [(Fr, Fr)] -> Bool
verifyDense (SRS h) circuit proof y z yzs = unsafePerformIO $
  withForeignPtr h $ \p -> withCircuit circuit $ \n q pwl pwr pwo pcs ->
    withBytes (encodeProof proof) $ \ppf -> withFr y $ \py -> withFr z $ \pz ->
      withFrs (concat [ [yj, zj] | (yj, zj) <- yzs ]) $ \pyz -> alloca $ \acc -> do
        check =<< c_verify p n q pwl pwr pwo pcs ppf py pz pyz acc
        (/= 0) <$> peek acc

-- | the opt-in Fiat-Shamir transcript's circuit digest (sonic_fs_circuit_digest_csr: host only, SHA-256 of the dense bytes the rows stand for)
fsCircuitDigest :: ArithCircuit Fr -> ByteString
fsCircuitDigest circuit = unsafePerformIO $
  withCircuitCsr circuit $ \n q prp pcol pval pcs -> BSI.create 32 $ \out ->
    check =<< c_fs_digest_csr n q prp pcol pval pcs out

-- | verify for a proof made with the Fiat-Shamir transcript (sonic_verify_fs_csr): the challenges are recomputed from circuit and proof
verifyFs :: SRS -> ArithCircuit Fr -> Proof -> Bool
verifyFs (SRS h) circuit proof = unsafePerformIO $
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \n q prp pcol pval pcs ->
    withBytes (encodeProof proof) $ \ppf -> alloca $ \acc -> do
      check =<< c_verify_fs_csr p n q prp pcol pval pcs ppf acc
      (/= 0) <$> peek acc

-- ---------------------------------------------------------------------------------------------------------------------
-- Sonic.Signature
-- ---------------------------------------------------------------------------------------------------------------------
-- | hscProve :: MonadRandom m => SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof   (src/Sonic/Signature.hs:32-72)
hscProve :: MonadRandom m => SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof
hscProve (SRS h) sXY yzs = do
  u <- rnd                              -- Signature.hs:48
  v <- rnd                              -- :60
  let m = length yzs
  pure $ unsafePerformIO $
    withForeignPtr h $ \p -> withBiTerms sXY $ \nt xs ys cs ->
      withFrs (concat [ [yj, zj] | (yj, zj) <- yzs ]) $ \pyz -> withFr u $ \pu -> withFr v $ \pv -> do
        sz <- fromIntegral <$> c_hsc_proof_size (fromIntegral m)
        bytes <- BSI.create sz $ \out ->
          check =<< c_hsc_prove_poly p nt xs ys cs (fromIntegral m) pyz pu pv out
        pure (decodeHscProof m bytes)

-- | hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool   (src/Sonic/Signature.hs:74-90)
hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool
hscVerify (SRS h) sXY yzs proof = unsafePerformIO $
  withForeignPtr h $ \p -> withBiTerms sXY $ \nt xs ys cs ->
    withFrs (concat [ [yj, zj] | (yj, zj) <- yzs ]) $ \pyz -> withBytes (encodeHscProof proof) $ \ph ->
      alloca $ \acc -> do
        check =<< c_hsc_verify_poly p nt xs ys cs (fromIntegral (length yzs)) pyz ph acc
        (/= 0) <$> peek acc

-- ---------------------------------------------------------------------------------------------------------------------
-- resident handles: circuit (and assignment) stay in HBM between proofs -- `mapM (prove srs asg) circuits` without re-uploading
-- ---------------------------------------------------------------------------------------------------------------------
data Prover = Prover { proverHandle :: ForeignPtr ProverHandle, proverSrs :: SRS, proverQ :: Int }

newProver :: SRS -> ArithCircuit Fr -> IO Prover
newProver srs@(SRS h) circuit =
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \n q prp pcol pval pcs -> alloca $ \out -> do
    check =<< c_prover_new_csr p n q prp pcol pval pcs out
    fp <- newForeignPtr p_prover_free =<< peek out
    pure Prover { proverHandle = fp, proverSrs = srs, proverQ = fromIntegral q }

-- | newProver over the dense Q x n weight arrays (sonic_prover_new): a handle that proves the same bytes
newProverDense :: SRS -> ArithCircuit Fr -> IO Prover
newProverDense srs@(SRS h) circuit =
  withForeignPtr h $ \p -> withCircuit circuit $ \n q pwl pwr pwo pcs -> alloca $ \out -> do
    check =<< c_prover_new p n q pwl pwr pwo pcs out
    fp <- newForeignPtr p_prover_free =<< peek out
    pure Prover { proverHandle = fp, proverSrs = srs, proverQ = fromIntegral q }       -- (keeps the SRS alive as long as the handle)

-- | once per circuit: commits the Q constraint rows of sPoly (Constraints.hs:34-53); same proof bytes afterwards, fewer terms
prepare :: Prover -> IO ()
prepare Prover{..} = withForeignPtr proverHandle (check <=< c_prover_prepare)

setAssignment :: Prover -> Assignment Fr -> IO ()
setAssignment Prover{..} Assignment{..} =
  withForeignPtr proverHandle $ \p -> withFrs aL $ \pal -> withFrs aR $ \par -> withFrs aO $ \pao ->
    check =<< c_prover_set p pal par pao

proofBytes :: Int -> (Ptr Word8 -> IO CInt) -> IO ByteString
proofBytes q body = do
  sz <- fromIntegral <$> c_proof_size (fromIntegral q)
  BSI.create sz (check <=< body)

-- | prove on a resident handle (Protocol.hs:47-109); the draws are made here exactly as `prove` makes them
proveWith :: Prover -> IO (Proof, RndOracle)
proveWith Prover{..} = do
  (transcript, oracle) <- drawTranscript proverQ
  bytes <- withForeignPtr proverHandle $ \p -> withFrs transcript $ \ptr ->
    proofBytes proverQ (c_prover_prove p ptr)
  pure (decodeProof proverQ bytes, oracle)

-- | the two halves of `proveWith`: `submit` queues the proof on the GPU and returns, `collect` waits and finishes it.  A thread that
--   alternates between two handles (submit a; submit b; collect a; submit a; collect b; ..) streams a list of proofs.
submit :: Prover -> IO RndOracle
submit Prover{..} = do
  (transcript, oracle) <- drawTranscript proverQ
  withForeignPtr proverHandle $ \p -> withFrs transcript $ \ptr -> check =<< c_prover_submit p ptr
  pure oracle

collect :: Prover -> IO Proof
collect Prover{..} =
  decodeProof proverQ <$> withForeignPtr proverHandle (\p -> proofBytes proverQ (c_prover_collect p))

withProvers :: [Prover] -> (Ptr (Ptr ProverHandle) -> CInt -> IO a) -> IO a
withProvers ps f = go ps []
  where
    go [] acc = let hs = reverse acc in allocaArray (length hs) $ \arr -> pokeArray arr hs >> f arr (fromIntegral (length hs))
    go (Prover{..} : rest) acc = withForeignPtr proverHandle $ \p -> go rest (p : acc)

-- | ONE proof made by several GPUs: handle r (on its own GPU, over a replica of the SRS, same circuit and assignment) runs rank r's
--   share of the proof's 7 + 4Q MSMs; same bytes as one GPU's proof
proveShared :: [Prover] -> IO (Proof, RndOracle)
proveShared [] = panic "proveShared: no handles"
proveShared ps@(p0 : _) = do
  let q = proverQ p0
  (transcript, oracle) <- drawTranscript q
  bytes <- withProvers ps $ \arr world -> withFrs transcript $ \ptr ->
    proofBytes q (c_prove_shared arr world ptr)
  pure (decodeProof q bytes, oracle)

-- | `mapM (\asg -> prove srs asg circuit) assignments` over the handles' GPUs (proof i on handle i mod length handles; two handles per
--   GPU stream that GPU's proofs); no collective
proveBatch :: [Prover] -> [Assignment Fr] -> IO [(Proof, RndOracle)]
proveBatch [] _ = panic "proveBatch: no handles"
proveBatch ps@(p0 : _) asgs = do
  let q = proverQ p0
      k = length asgs
  drawn <- replicateM k (drawTranscript q)
  psz <- fromIntegral <$> c_proof_size (fromIntegral q)
  bytes <- withProvers ps $ \arr np ->
    withFrs (concatMap aL asgs) $ \pal -> withFrs (concatMap aR asgs) $ \par -> withFrs (concatMap aO asgs) $ \pao ->
      withFrs (concatMap fst drawn) $ \ptr ->
        BSI.create (psz * k) $ \out ->
          check =<< c_prove_batch arr np (fromIntegral k) pal par pao ptr out nullPtr
  pure (zip (map (decodeProof q) (chunks psz bytes)) (map snd drawn))

-- ---------------------------------------------------------------------------------------------------------------------
-- one circuit, many statements: the weights are the program and stay resident, the constants cs = wL.aL + wR.aR + wO.aO
-- (test/Test/Reference.hs:138) are the public inputs and change with every proof
-- ---------------------------------------------------------------------------------------------------------------------
-- | the constants of the handle's next statement, overwritten in place (sonic_prover_set_constants): assignment and prepared rows stay
setConstants :: Prover -> [Fr] -> IO ()
setConstants Prover{..} cs
  | length cs /= proverQ = panic "setConstants: need Q constants"
  | otherwise = withForeignPtr proverHandle $ \p -> withFrs cs (check <=< c_set_constants p)

-- | per assignment: the constants it satisfies under the handle's weights, and (broken multiplication gates, the first one or -1), on the
--   GPU (sonic_prover_eval_constraints)
evalConstraints :: Prover -> [Assignment Fr] -> IO [([Fr], (Int, Int))]
evalConstraints _ [] = pure []
evalConstraints Prover{..} asgs = do
  let b = length asgs
  withForeignPtr proverHandle $ \p ->
    withFrs (concatMap aL asgs) $ \pal -> withFrs (concatMap aR asgs) $ \par -> withFrs (concatMap aO asgs) $ \pao ->
      allocaArray (2 * b) $ \gates -> do
        bytes <- BSI.create (32 * proverQ * b) $ \out ->
          check =<< c_eval_constraints p (fromIntegral b) pal par pao out gates
        gs <- forM [0 .. b - 1] $ \i -> (,) <$> peekElemOff gates (2 * i) <*> peekElemOff gates (2 * i + 1)
        pure [ (map frFromBytes (chunks 32 one), (fromIntegral c, fromIntegral f)) | (one, (c, f)) <- zip (chunks (32 * proverQ) bytes) gs ]

-- | proveBatch with one statement per proof (sonic_prove_batch_statements): proof i's constants ride at the head of its own queue as its
--   assignment does.  Afterwards each handle holds the constants and the assignment of the last proof it ran.
proveBatchStatements :: [Prover] -> [(Assignment Fr, [Fr])] -> IO [(Proof, RndOracle)]
proveBatchStatements [] _ = panic "proveBatchStatements: no handles"
proveBatchStatements ps@(p0 : _) sts = do
  let q = proverQ p0
      k = length sts
      asgs = map fst sts
  when (any ((/= q) . length . snd) sts) $ panic "proveBatchStatements: need Q constants per statement"
  drawn <- replicateM k (drawTranscript q)
  psz <- fromIntegral <$> c_proof_size (fromIntegral q)
  bytes <- withProvers ps $ \arr np ->
    withFrs (concatMap aL asgs) $ \pal -> withFrs (concatMap aR asgs) $ \par -> withFrs (concatMap aO asgs) $ \pao ->
      withFrs (concatMap snd sts) $ \pcs -> withFrs (concatMap fst drawn) $ \ptr ->
        BSI.create (psz * k) $ \out ->
          check =<< c_prove_batch_st arr np (fromIntegral k) pal par pao pcs ptr out nullPtr
  pure (zip (map (decodeProof q) (chunks psz bytes)) (map snd drawn))

-- | the SHA-256 state of the circuit digest after the gate weights (sonic_fs_circuit_midstate_csr; host only): 112 bytes
fsCircuitMidstate :: ArithCircuit Fr -> ByteString
fsCircuitMidstate circuit = unsafePerformIO $
  withCircuitCsr circuit $ \n q prp pcol pval _ -> BSI.create 112 $ \out ->
    check =<< c_fs_midstate_csr n q prp pcol pval out

-- | fsCircuitDigest of the circuit behind the midstate with these constants, from Q x 32 bytes of hashing
fsCircuitDigestResume :: ByteString -> [Fr] -> ByteString
fsCircuitDigestResume mid cs = unsafePerformIO $
  withBytes mid $ \pm -> withFrs cs $ \pcs -> BSI.create 32 $ \out ->
    check =<< c_fs_resume pm pcs out

-- ---------------------------------------------------------------------------------------------------------------------
-- Fiat-Shamir proofs in flight: the six passes of a Fiat-Shamir proof walked by a host thread the handle owns, so that one Haskell thread
-- keeps several handles busy; the blinders come from witness digest v2, which the GPU computes over the resident assignment
-- ---------------------------------------------------------------------------------------------------------------------
-- the handle for the duration of a call, and with it the SRS it proves over
withProverAlive :: Prover -> (Ptr ProverHandle -> IO a) -> IO a
withProverAlive Prover{..} f = case proverSrs of SRS h -> withForeignPtr h $ \_ -> withForeignPtr proverHandle f

-- | witness digest v2 of the resident assignment (sonic_prover_witness_digest_v2): 32 bytes
witnessDigest :: Prover -> IO ByteString
witnessDigest pr = withProverAlive pr $ \p -> BSI.create 32 (check <=< c_witness_digest p)

-- | hand one Fiat-Shamir proof to the handle and return (sonic_prover_submit_fs): circuit digest (fsCircuitDigest, or
--   fsCircuitDigestResume after setConstants) and the prover's secret 32-byte blinder seed
submitFs :: Prover -> ByteString -> ByteString -> IO ()
submitFs pr digest seed
  | BS.length digest /= 32 || BS.length seed /= 32 = panic "submitFs: the circuit digest and the seed are 32 bytes each"
  | otherwise = withProverAlive pr $ \p -> withBytes digest $ \pd -> withBytes seed $ \ps -> check =<< c_prover_submit_fs p pd ps

-- | wait for the proof `submitFs` started (sonic_prover_collect_fs): the proof and the 8 + 2Q transcript values it was made with
collectFs :: Prover -> IO (Proof, [Fr])
collectFs pr@Prover{..} = withProverAlive pr $ \p -> do
  let tsz = 32 * (8 + 2 * proverQ)
  allocaBytes tsz $ \ptr -> do
    bytes <- proofBytes proverQ (\out -> c_prover_collect_fs p out ptr)
    tr <- BS.packCStringLen (castPtr ptr, tsz)
    pure (decodeProof proverQ bytes, map frFromBytes (chunks 32 tr))

-- | K Fiat-Shamir proofs over the handles' GPUs (sonic_prove_batch_fs; proof i on handle i mod length handles): per proof its
--   assignment, its constants, its circuit digest (fsCircuitDigestResume midstate constants) and its blinder seed
proveBatchFs :: [Prover] -> [(Assignment Fr, [Fr], ByteString, ByteString)] -> IO [Proof]
proveBatchFs [] _ = panic "proveBatchFs: no handles"
proveBatchFs ps@(p0 : _) sts = do
  let q = proverQ p0
      k = length sts
      asgs = [ a | (a, _, _, _) <- sts ]
  when (any (\(_, cs, dg, sd) -> length cs /= q || BS.length dg /= 32 || BS.length sd /= 32) sts) $
    panic "proveBatchFs: need Q constants, a 32-byte digest and a 32-byte seed per statement"
  psz <- fromIntegral <$> c_proof_size (fromIntegral q)
  bytes <- withProverAlive p0 $ \_ -> withProvers ps $ \arr np ->
    withFrs (concatMap aL asgs) $ \pal -> withFrs (concatMap aR asgs) $ \par -> withFrs (concatMap aO asgs) $ \pao ->
      withFrs (concat [ cs | (_, cs, _, _) <- sts ]) $ \pcs ->
        withBytes (BS.concat [ dg | (_, _, dg, _) <- sts ]) $ \pdg -> withBytes (BS.concat [ sd | (_, _, _, sd) <- sts ]) $ \psd ->
          BSI.create (psz * k) $ \out ->
            check =<< c_prove_batch_fs arr np (fromIntegral k) pal par pao pcs pdg psd out nullPtr nullPtr
  pure (map (decodeProof q) (chunks psz bytes))

-- ---------------------------------------------------------------------------------------------------------------------
-- witness sources (include/sonic_hip.h, "Witness sources"): host or device memory, 32-byte canonical Fr or int64, aO given or derived.
-- The source is only read and must stay unchanged until the call returns; every call is blocking.  A non-NULL stream of a device
-- source is the stream whose work produces the data: the library records an event on it at entry and the handle's stream waits on
-- that event; NULL states that the data is complete.
-- ---------------------------------------------------------------------------------------------------------------------
-- | sonic_witness_src_t: 48 bytes -- aL, aR, aO at 0, 8, 16; kind, on_device (int32) at 24, 28; stride (int64) at 32; hip_stream at 40
data WitnessSrc = WitnessSrc
  { wsAL, wsAR, wsAO :: Ptr ()       -- ^ wsAO = nullPtr: the library sets aO = aL * aR in Fr
  , wsKind     :: Int32              -- ^ 0 = SONIC_WIT_FR32 (32-byte canonical Fr), 1 = SONIC_WIT_I64 (v < 0 is r - |v|)
  , wsOnDevice :: Int32              -- ^ 0: host memory; 1: memory of the GPU the handle lives on
  , wsStride   :: Int64              -- ^ bytes from assignment b to b + 1 in batched calls; 0 = packed
  , wsStream   :: Ptr ()             -- ^ device sources only: the producing stream, or nullPtr
  }

instance Storable WitnessSrc where
  sizeOf _    = 48
  alignment _ = 8
  peek p = WitnessSrc <$> peekByteOff p 0 <*> peekByteOff p 8 <*> peekByteOff p 16 <*> peekByteOff p 24 <*> peekByteOff p 28
                      <*> peekByteOff p 32 <*> peekByteOff p 40
  poke p WitnessSrc{..} = do
    pokeByteOff p 0 wsAL; pokeByteOff p 8 wsAR; pokeByteOff p 16 wsAO
    pokeByteOff p 24 wsKind; pokeByteOff p 28 wsOnDevice; pokeByteOff p 32 wsStride; pokeByteOff p 40 wsStream

-- a host source of int64 with aO derived
hostI64 :: Ptr Int64 -> Ptr Int64 -> WitnessSrc
hostI64 pl pr = WitnessSrc { wsAL = castPtr pl, wsAR = castPtr pr, wsAO = nullPtr, wsKind = 1, wsOnDevice = 0, wsStride = 0, wsStream = nullPtr }

-- | the handle's assignment from machine integers (sonic_prover_set_witness): aL, aR as int64, aO = aL * aR formed on the GPU; 8 n bytes
--   per vector cross the bus instead of 32 n, and nothing is widened on the host
setWitnessI64 :: Prover -> [Int64] -> [Int64] -> IO ()
setWitnessI64 pr ls rs
  | length ls /= length rs = panic "setWitnessI64: aL and aR differ in length"
  | otherwise = withProverAlive pr $ \p -> withArray ls $ \pl -> withArray rs $ \prr ->
      with (hostI64 pl prr) $ \src -> check =<< c_prover_set_witness p src

-- | proveBatch over assignments given as (aL, aR) in machine integers (sonic_prove_batch_src; the handles' constants): proof i reads
--   block i of the two packed arrays, converted at the head of its own queue
proveBatchI64 :: [Prover] -> [([Int64], [Int64])] -> IO [(Proof, RndOracle)]
proveBatchI64 [] _ = panic "proveBatchI64: no handles"
proveBatchI64 ps@(p0 : _) asgs = do
  let q = proverQ p0
      k = length asgs
      n = case asgs of { ((l, _) : _) -> length l; [] -> 0 }
  when (any (\(l, r) -> length l /= n || length r /= n) asgs) $ panic "proveBatchI64: every assignment needs n values in aL and in aR"
  drawn <- replicateM k (drawTranscript q)
  psz <- fromIntegral <$> c_proof_size (fromIntegral q)
  bytes <- withProverAlive p0 $ \_ -> withProvers ps $ \arr np ->
    withArray (concatMap fst asgs) $ \pl -> withArray (concatMap snd asgs) $ \prr ->
      with (hostI64 pl prr) $ \src -> withFrs (concatMap fst drawn) $ \ptr ->
        BSI.create (psz * k) $ \out ->
          check =<< c_prove_batch_src arr np (fromIntegral k) src nullPtr ptr out nullPtr
  pure (zip (map (decodeProof q) (chunks psz bytes)) (map snd drawn))

-- ---------------------------------------------------------------------------------------------------------------------
-- R1CS front end (include/sonic_hip.h, "R1CS front end"): three CSR matrices A, B, C with <A_i, z> <B_i, z> = <C_i, z>, column 0 the
-- constant one and columns 1..nPub the public inputs, compiled under layout 1 to a Sonic constraint system of n = m + N / 2 gates and
-- Q = 3m + nPub linear constraints.  Prove such circuits with core proofs: Q is of the order of n.
-- ---------------------------------------------------------------------------------------------------------------------
data R1csHandle

-- | sonic_r1cs_matrix_t: 24 bytes -- row_ptr (m + 1 int64), col (int64), val (32-byte canonical Fr) at 0, 8, 16
data R1csMatrix = R1csMatrix { rmRowPtr :: Ptr Int64, rmCol :: Ptr Int64, rmVal :: Ptr Word8 }

instance Storable R1csMatrix where
  sizeOf _    = 24
  alignment _ = 8
  peek p = R1csMatrix <$> peekByteOff p 0 <*> peekByteOff p 8 <*> peekByteOff p 16
  poke p R1csMatrix{..} = do pokeByteOff p 0 rmRowPtr; pokeByteOff p 8 rmCol; pokeByteOff p 16 rmVal

-- | the handle and its shape: gates, linear constraints, entries of the Sonic CSR, variable gates
data R1CS = R1CS { r1csHandle :: ForeignPtr R1csHandle, r1csN, r1csQ, r1csNnz, r1csG :: Int }

-- | sonic_r1cs_new over rows given as [(column, coefficient)] with strictly increasing columns
newR1cs :: Int -> Int -> [[(Int, Fr)]] -> [[(Int, Fr)]] -> [[(Int, Fr)]] -> IO R1CS
newR1cs bigN nPub as bs cs = libraryReady `seq` withMat as (\pa -> withMat bs (\pb -> withMat cs (\pc -> alloca $ \out -> allocaArray 4 $ \shp -> do
    check =<< c_r1cs_new (fromIntegral (length as)) (fromIntegral bigN) (fromIntegral nPub) pa pb pc out
    fp <- newForeignPtr p_r1cs_free =<< peek out
    withForeignPtr fp $ \h -> check =<< c_r1cs_shape h shp
    [n, q, z, g] <- map fromIntegral <$> mapM (peekElemOff shp) [0 .. 3 :: Int]
    pure R1CS { r1csHandle = fp, r1csN = n, r1csQ = q, r1csNnz = z, r1csG = g })))
  where
    withMat :: [[(Int, Fr)]] -> (Ptr R1csMatrix -> IO a) -> IO a
    withMat rows f =
      withArray (scanl (+) 0 (map (fromIntegral . length) rows) :: [Int64]) $ \prp ->
        withArray (map (fromIntegral . fst) (concat rows) :: [Int64]) $ \pcol ->
          withFrs (map snd (concat rows)) $ \pval -> with (R1csMatrix prp pcol pval) f

-- | the compiled Sonic CSR (sonic_r1cs_circuit): row_ptr (3Q + 1), col, val, and the constants with the public slots zero
r1csCircuit :: R1CS -> IO ([Int64], [Int64], [Fr], [Fr])
r1csCircuit R1CS{..} = withForeignPtr r1csHandle $ \h ->
  allocaArray (3 * r1csQ + 1) $ \prp -> allocaArray (max 1 r1csNnz) $ \pcol ->
   allocaBytes (32 * max 1 r1csNnz) $ \pval -> allocaBytes (32 * r1csQ) $ \pcs -> do
    check =<< c_r1cs_circuit h prp pcol pval pcs
    vb <- BS.packCStringLen (castPtr pval, 32 * r1csNnz)
    csb <- BS.packCStringLen (castPtr pcs, 32 * r1csQ)
    rp <- mapM (peekElemOff prp) [0 .. 3 * r1csQ]
    cl <- mapM (peekElemOff pcol) [0 .. r1csNnz - 1]
    pure (rp, cl, map frFromBytes (take r1csNnz (chunks 32 vb)), map frFromBytes (chunks 32 csb))

-- | K witnesses of N machine integers each, on the host (sonic_r1cs_assign, SONIC_WIT_I64): the planes are written to three device
--   buffers of K n 32 bytes on the handle's GPU, packed; the result is each witness's constants and its (broken gates, first or -1)
r1csAssignI64 :: R1CS -> [[Int64]] -> Ptr () -> Ptr () -> Ptr () -> IO [([Fr], (Int64, Int64))]
r1csAssignI64 R1CS{..} zs dL dR dO = withForeignPtr r1csHandle $ \h -> do
  let k = length zs
  withArray (concat zs) $ \pz -> allocaArray (2 * k) $ \pbad -> do
    csb <- BSI.create (32 * r1csQ * k) $ \pcs ->
      check =<< c_r1cs_assign h (fromIntegral k) (castPtr pz) 1 0 0 nullPtr dL dR dO 0 pcs pbad
    bad <- mapM (peekElemOff pbad) [0 .. 2 * k - 1]
    let pairs (a : b : r) = (a, b) : pairs r
        pairs _ = []
    pure (zip (map (map frFromBytes . chunks 32) (chunks (32 * r1csQ) csb)) (pairs bad))

-- | the batched verifier's handle (sonic_verifier_new_csr): the circuit resident on the GPU; keeps the SRS alive as long as the handle
data Verifier = Verifier { verifierHandle :: ForeignPtr VerifierHandle, verifierSrs :: SRS, verifierQ :: Int }

newVerifier :: SRS -> ArithCircuit Fr -> IO Verifier
newVerifier srs@(SRS h) circuit =
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \n q prp pcol pval pcs -> alloca $ \out -> do
    check =<< c_verifier_new_csr p n q prp pcol pval pcs out
    fp <- newForeignPtr p_verifier_free =<< peek out
    pure Verifier { verifierHandle = fp, verifierSrs = srs, verifierQ = fromIntegral q }

-- ---------------------------------------------------------------------------------------------------------------------
-- Circuits with Q ~ n: weights digest v2 and circuit digest v2 hash the CSR ENTRIES (a SHA-256 tree, O(nnz)) where v1 hashes the
-- 96 Q n dense bytes; an explicit zero is an entry.  The prover's Fiat-Shamir calls take the digest they are given, so proofs for a
-- verifier of digest kind 2 are made under fsCircuitDigestV2 (proveCoreFs, submitFs) and aggregates under the v2 weights digest.
-- ---------------------------------------------------------------------------------------------------------------------
-- | weights digest v2 of the circuit's CSR (sonic_fs_weights_digest_v2_csr; host only): 32 bytes
fsWeightsDigestV2 :: ArithCircuit Fr -> ByteString
fsWeightsDigestV2 circuit = unsafePerformIO $
  withCircuitCsr circuit $ \n q prp pcol pval _ -> BSI.create 32 $ \out ->
    check =<< c_fs_weights_digest_v2 n q prp pcol pval out

-- | circuit digest v2 of one statement (sonic_fs_circuit_digest_v2; host only): weights digest v2, then the constants
fsCircuitDigestV2 :: ByteString -> [Fr] -> ByteString
fsCircuitDigestV2 wd cs = unsafePerformIO $
  withBytes wd $ \pw -> withFrs cs $ \pcs -> BSI.create 32 $ \out ->
    check =<< c_fs_circuit_digest_v2 pw (fromIntegral (length cs)) pcs out

-- | weights digest v2 from the prover handle's resident CSR, computed on the GPU (sonic_prover_weights_digest_v2)
proverWeightsDigestV2 :: Prover -> IO ByteString
proverWeightsDigestV2 pr = withProverAlive pr $ \p -> BSI.create 32 (check <=< c_prover_weights_digest_v2 p)

-- | the same from a verifier handle (sonic_verifier_weights_digest_v2)
verifierWeightsDigestV2 :: Verifier -> IO ByteString
verifierWeightsDigestV2 Verifier{..} = withForeignPtr verifierHandle $ \v -> BSI.create 32 (check <=< c_verifier_weights_digest_v2 v)

-- | newVerifier with the digest kind chosen (sonic_verifier_new_digest): 1 is newVerifier; 2 derives circuit digest v2 and hashes
--   nothing dense when the handle is made
newVerifierDigest :: Int -> SRS -> ArithCircuit Fr -> IO Verifier
newVerifierDigest kind srs@(SRS h) circuit =
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \n q prp pcol pval pcs -> alloca $ \out -> do
    check =<< c_verifier_new_digest p n q prp pcol pval pcs (fromIntegral kind) out
    fp <- newForeignPtr p_verifier_free =<< peek out
    pure Verifier { verifierHandle = fp, verifierSrs = srs, verifierQ = fromIntegral q }

-- | 1 or 2 (sonic_verifier_digest_kind)
verifierDigestKind :: Verifier -> IO Int
verifierDigestKind Verifier{..} = withForeignPtr verifierHandle $ \v -> fromIntegral <$> c_verifier_digest_kind v

-- | the device memory the prover handle owns now (sonic_prover_device_bytes): the signature's state (MSM slots 5 and above, the pairs'
--   buffers) appears with the first full proof
proverDeviceBytes :: Prover -> IO Int64
proverDeviceBytes pr = withProverAlive pr $ \p -> alloca $ \out -> do
  check =<< c_prover_device_bytes p out
  peek out

-- | the pinned host memory the prover handle owns now (sonic_prover_host_bytes): a core proof's staging until the first proof with a
--   signature, whose MSM slots (5 Q + 8 of 12 304 bytes) then appear here and on the device
proverHostBytes :: Prover -> IO Int64
proverHostBytes pr = withProverAlive pr $ \p -> alloca $ \out -> do
  check =<< c_prover_host_bytes p out
  peek out

-- | K proofs of K statements of the handle's circuit in one pairing product (sonic_verifier_verify_batch_cs): proof k against cs_k with
--   its RndOracle; the per-proof verdicts (a malformed proof is a rejected proof).  The library draws the seed of the randomizers.
verifyBatchStatements :: Verifier -> [(Proof, RndOracle, [Fr])] -> IO [Bool]
verifyBatchStatements _ [] = pure []
verifyBatchStatements Verifier{..} sts = do
  let k = length sts
      chal RndOracle{..} = rndOracleY : rndOracleZ : concat [ [yj, zj] | (yj, zj) <- rndOracleYZs ]
  withForeignPtr verifierHandle $ \v ->
    withBytes (BS.concat [ encodeProof pf | (pf, _, _) <- sts ]) $ \ppf ->
      withFrs (concat [ chal o | (_, o, _) <- sts ]) $ \pch -> withFrs (concat [ cs | (_, _, cs) <- sts ]) $ \pcs ->
        alloca $ \acc -> do
          each <- BSI.create k $ \out -> check =<< c_verify_batch_cs v (fromIntegral k) ppf 0 pch pcs nullPtr acc out
          pure (map (/= 0) (BS.unpack each))

-- | the same for Fiat-Shamir proofs (sonic_verifier_verify_fs_batch_cs): proof k's challenges come from the digest of its own statement
verifyFsBatchStatements :: Verifier -> [(Proof, [Fr])] -> IO [Bool]
verifyFsBatchStatements _ [] = pure []
verifyFsBatchStatements Verifier{..} sts = do
  let k = length sts
  withForeignPtr verifierHandle $ \v ->
    withBytes (BS.concat (map (encodeProof . fst) sts)) $ \ppf -> withFrs (concatMap snd sts) $ \pcs ->
      alloca $ \acc -> do
        each <- BSI.create k $ \out -> check =<< c_verify_fs_batch_cs v (fromIntegral k) ppf 0 pcs nullPtr acc out
        pure (map (/= 0) (BS.unpack each))

-- ---------------------------------------------------------------------------------------------------------------------
-- core proofs (include/sonic_hip.h, "Core proofs"): the head of a `Proof` -- R, T, a, W_a, b, W_b, W_t, s -- and no signature.  Nothing
-- that `verify` checks ties a proof's s to s(z, y); `verifyCore` evaluates s(z, y) itself, rejects a proof whose s differs and checks
-- the three pcV equations of the head.  `verifyCore srs circuit (coreOf proof) y z` is the sound check of an existing full proof.
-- ---------------------------------------------------------------------------------------------------------------------
data CoreProof = CoreProof
  { cpR :: G1 BLS12381, cpT :: G1 BLS12381, cpA :: Fr, cpWa :: G1 BLS12381, cpB :: Fr, cpWb :: G1 BLS12381, cpWt :: G1 BLS12381, cpS :: Fr }

-- | the head of a full proof
coreOf :: Proof -> CoreProof
coreOf Proof{..} = CoreProof { cpR = prR, cpT = prT, cpA = prA, cpWa = prWa, cpB = prB, cpWb = prWb, cpWt = prWt, cpS = prS }

-- | 5 G1 + 3 Fr = 576 bytes, whatever Q is
decodeCoreProof :: ByteString -> CoreProof
decodeCoreProof b0 =
  let (r, b1)  = takeG b0
      (t, b2)  = takeG b1
      (a, b3)  = takeF b2
      (wa, b4) = takeG b3
      (b, b5)  = takeF b4
      (wb, b6) = takeG b5
      (wt, b7) = takeG b6
      (s, _)   = takeF b7
  in CoreProof { cpR = r, cpT = t, cpA = a, cpWa = wa, cpB = b, cpWb = wb, cpWt = wt, cpS = s }

encodeCoreProof :: CoreProof -> ByteString
encodeCoreProof CoreProof{..} = BS.concat
  [ g1ToBytes cpR, g1ToBytes cpT, frToBytes cpA, g1ToBytes cpWa, frToBytes cpB, g1ToBytes cpWb, g1ToBytes cpWt, frToBytes cpS ]

coreProofSize :: Int
coreProofSize = 576

-- the four blinders and y, z, drawn in the order `prove` draws them (Protocol.hs:58,66,76)
drawCoreTranscript :: MonadRandom m => m ([Fr], (Fr, Fr))
drawCoreTranscript = do
  cns <- replicateM 4 rnd
  y   <- rnd
  z   <- rnd
  pure (cns ++ [y, z], (y, z))

-- | a core proof on a resident handle (sonic_prover_prove_core) and the (y, z) it was made at: the head of what `proveWith` would give
--   for the same draws, from 5 MSMs instead of 7 + 4Q
proveCore :: Prover -> IO (CoreProof, (Fr, Fr))
proveCore pr = do
  (transcript, yz) <- drawCoreTranscript
  bytes <- withProverAlive pr $ \p -> withFrs transcript $ \ptr ->
    BSI.create coreProofSize (check <=< c_prover_prove_core p ptr)
  pure (decodeCoreProof bytes, yz)

-- | the two halves of `proveCore`, as `submit` / `collect`
submitCore :: Prover -> IO (Fr, Fr)
submitCore pr = do
  (transcript, yz) <- drawCoreTranscript
  withProverAlive pr $ \p -> withFrs transcript $ \ptr -> check =<< c_prover_submit_core p ptr
  pure yz

collectCore :: Prover -> IO CoreProof
collectCore pr = decodeCoreProof <$> withProverAlive pr (\p -> BSI.create coreProofSize (check <=< c_prover_collect_core p))

-- | a core proof under its own Fiat-Shamir transcript (sonic_prover_prove_core_fs; label "sonic-hip/fs-core/v1"): circuit digest and
--   the prover's secret 32-byte blinder seed in, the proof and its (y, z) out
proveCoreFs :: Prover -> ByteString -> ByteString -> IO (CoreProof, (Fr, Fr))
proveCoreFs pr digest seed
  | BS.length digest /= 32 || BS.length seed /= 32 = panic "proveCoreFs: the circuit digest and the seed are 32 bytes each"
  | otherwise = withProverAlive pr $ \p -> withBytes digest $ \pd -> withBytes seed $ \ps -> allocaBytes 64 $ \pyz -> do
      bytes <- BSI.create coreProofSize (\out -> check =<< c_prover_prove_core_fs p pd ps out pyz)
      yz <- BS.packCStringLen (castPtr pyz, 64)
      pure (decodeCoreProof bytes, (frFromBytes (BS.take 32 yz), frFromBytes (BS.drop 32 yz)))

-- | the sound check of a proof's head (sonic_verify_core_csr): False when the proof's s is not s(z, y) or one of the three equations fails
verifyCore :: SRS -> ArithCircuit Fr -> CoreProof -> Fr -> Fr -> Bool
verifyCore (SRS h) circuit proof y z = unsafePerformIO $
  withForeignPtr h $ \p -> withCircuitCsr circuit $ \n q prp pcol pval pcs ->
    withBytes (encodeCoreProof proof) $ \ppf -> withFr y $ \py -> withFr z $ \pz -> alloca $ \acc -> do
      check =<< c_verify_core_csr p n q prp pcol pval pcs ppf py pz acc
      (/= 0) <$> peek acc

-- | K core proofs of K statements of the handle's circuit in one pairing product (sonic_verifier_verify_core_batch): proof k at its
--   (y, z) against cs_k; the per-proof verdicts.  A proof whose s is not s(z_k, y_k) is a rejected proof.
verifyCoreBatch :: Verifier -> [(CoreProof, (Fr, Fr), [Fr])] -> IO [Bool]
verifyCoreBatch _ [] = pure []
verifyCoreBatch Verifier{..} sts = do
  let k = length sts
  withForeignPtr verifierHandle $ \v ->
    withBytes (BS.concat [ encodeCoreProof pf | (pf, _, _) <- sts ]) $ \ppf ->
      withFrs (concat [ [y, z] | (_, (y, z), _) <- sts ]) $ \pyz -> withFrs (concat [ cs | (_, _, cs) <- sts ]) $ \pcs ->
        alloca $ \acc -> do
          each <- BSI.create k $ \out -> check =<< c_verify_core_batch v (fromIntegral k) ppf 0 pyz pcs nullPtr acc out
          pure (map (/= 0) (BS.unpack each))

-- | SHA-256 of the gate weights alone (sonic_fs_weights_digest over fsCircuitMidstate): what the transcript of an aggregate binds, since
--   s(X, Y) does not depend on the constants
fsWeightsDigest :: ArithCircuit Fr -> ByteString
fsWeightsDigest circuit = unsafePerformIO $
  withBytes (fsCircuitMidstate circuit) $ \pm -> BSI.create 32 $ \out -> check =<< c_fs_weights_digest pm out

-- | the helper of helped verification (sonic_prover_aggregate_core): ONE signature of correct computation over the (y_k, z_k) of K core
--   proofs of the handle's circuit -- an HscProof with m = K whose s_k is s(z_k, y_k), and whose u, v come from the aggregate's own
--   transcript under the weights digest (fsWeightsDigest of the circuit)
aggregateCore :: Prover -> ByteString -> [(Fr, Fr)] -> IO HscProof
aggregateCore pr wdigest yzs
  | BS.length wdigest /= 32 = panic "aggregateCore: a weights digest is 32 bytes"
  | null yzs = panic "aggregateCore: at least one (y, z) pair"
  | otherwise = withProverAlive pr $ \p -> withBytes wdigest $ \pw -> withFrs (concat [ [y, z] | (y, z) <- yzs ]) $ \pyz -> do
      let k = length yzs
      sz <- fromIntegral <$> c_hsc_proof_size (fromIntegral k)
      bytes <- BSI.create sz $ \out -> check =<< c_prover_aggregate_core p pw (fromIntegral k) pyz out
      pure (decodeHscProof k bytes)

-- | verifyCoreBatch with a helper's aggregate over the same (y, z) (sonic_verifier_verify_core_batch_helped): proof k's s is held against
--   the aggregate's s_k and s(u, v) is evaluated once per batch.  An aggregate that is malformed, not under its own transcript, or whose
--   global check fails rejects every proof.
verifyCoreBatchHelped :: Verifier -> [(CoreProof, (Fr, Fr), [Fr])] -> HscProof -> IO [Bool]
verifyCoreBatchHelped _ [] _ = pure []
verifyCoreBatchHelped Verifier{..} sts agg = do
  let k = length sts
  withForeignPtr verifierHandle $ \v ->
    withBytes (BS.concat [ encodeCoreProof pf | (pf, _, _) <- sts ]) $ \ppf ->
      withFrs (concat [ [y, z] | (_, (y, z), _) <- sts ]) $ \pyz -> withFrs (concat [ cs | (_, _, cs) <- sts ]) $ \pcs ->
        withBytes (encodeHscProof agg) $ \pagg -> alloca $ \acc -> do
          each <- BSI.create k $ \out -> check =<< c_verify_core_batch_helped v (fromIntegral k) ppf 0 pyz pcs pagg nullPtr acc out
          pure (map (/= 0) (BS.unpack each))

deviceCount :: IO Int
deviceCount = alloca $ \out -> do
  _ <- c_device_count out                -- (SONIC_ERR_NO_DEVICE and 0 without a GPU: there is no CPU fallback)
  fromIntegral <$> peek out
