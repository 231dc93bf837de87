//! `KzgProof` of kzg-rs `src/kzg_proof.rs:350-526`: the four verification functions with their signatures, early
//! returns and error variants; each forwards to one entry point of the library.
use crate::dtypes::{Blob, Bytes32, Bytes48, Cell};
use crate::enums::KzgError;
use crate::ffi;
use crate::trusted_setup::KzgSettings;
use alloc::{string::ToString, vec::Vec};
use bls12_381::{G1Affine, Scalar};

pub struct KzgProof {}

impl KzgProof {
    /// kzg-rs `src/kzg_proof.rs:353-397`.
    pub fn verify_kzg_proof(
        commitment_bytes: &Bytes48,
        z_bytes: &Bytes32,
        y_bytes: &Bytes32,
        proof_bytes: &Bytes48,
        kzg_settings: &KzgSettings,
    ) -> Result<bool, KzgError> {
        let mut ok = false;
        ffi::check(unsafe {
            ffi::kzg_verify_kzg_proof(&mut ok, commitment_bytes.0.as_ptr(), z_bytes.0.as_ptr(), y_bytes.0.as_ptr(), proof_bytes.0.as_ptr(), kzg_settings.raw())
        })?;
        Ok(ok)
    }

    /// kzg-rs `src/kzg_proof.rs:399-444`: typed inputs; they cross the C ABI as compressed points and big-endian
    /// canonical scalars.  Slices shorter than `commitments` index out of bounds in the reference: a panic here too.
    pub fn verify_kzg_proof_batch(
        commitments: &[G1Affine],
        zs: &[Scalar],
        ys: &[Scalar],
        proofs: &[G1Affine],
        kzg_settings: &KzgSettings,
    ) -> Result<bool, KzgError> {
        let n = commitments.len();
        let (zs, ys, proofs) = (&zs[..n], &ys[..n], &proofs[..n]);
        let be = |s: &Scalar| {
            let mut b = s.to_bytes();
            b.reverse();
            b
        };
        let c: Vec<u8> = commitments.iter().flat_map(|p| p.to_compressed()).collect();
        let p: Vec<u8> = proofs.iter().flat_map(|p| p.to_compressed()).collect();
        let z: Vec<u8> = zs.iter().flat_map(be).collect();
        let y: Vec<u8> = ys.iter().flat_map(be).collect();
        let mut ok = false;
        ffi::check(unsafe { ffi::kzg_verify_kzg_proof_batch(&mut ok, c.as_ptr(), z.as_ptr(), y.as_ptr(), p.as_ptr(), n, kzg_settings.raw()) })?;
        Ok(ok)
    }

    /// Not in kzg-rs: n independent `verify_kzg_proof` calls (`src/kzg_proof.rs:353-397`) through one library call, each
    /// proof with its own pairing and its own result - what a caller looping over `verify_kzg_proof` (the revm point
    /// evaluation precompile, one call per transaction) would write.  Entry i is what `verify_kzg_proof` returns for
    /// tuple i.  The four slices must have equal lengths.
    pub fn verify_kzg_proofs(
        commitment_bytes: &[Bytes48],
        zs: &[Bytes32],
        ys: &[Bytes32],
        proof_bytes: &[Bytes48],
        kzg_settings: &KzgSettings,
    ) -> Result<Vec<Result<bool, KzgError>>, KzgError> {
        let n = commitment_bytes.len();
        if zs.len() != n || ys.len() != n || proof_bytes.len() != n {
            return Err(KzgError::InvalidBytesLength("verify_kzg_proofs: slices of unequal length".to_string()));
        }
        let mut ok = vec![false; n];
        let mut err = vec![0u8; n];
        // (`Bytes32` / `Bytes48` are `repr(transparent)` byte arrays: the slices are handed over as they lie in memory)
        ffi::check(unsafe {
            ffi::kzg_verify_kzg_proofs(
                ok.as_mut_ptr(),
                err.as_mut_ptr(),
                commitment_bytes.as_ptr() as *const u8,
                zs.as_ptr() as *const u8,
                ys.as_ptr() as *const u8,
                proof_bytes.as_ptr() as *const u8,
                n,
                kzg_settings.raw(),
            )
        })?;
        Ok((0..n)
            .map(|i| if err[i] != 0 { Err(KzgError::BadArgs("Failed to parse G1Affine from bytes".to_string())) } else { Ok(ok[i]) })
            .collect())
    }

    /// kzg-rs `src/kzg_proof.rs:446-470`.
    pub fn verify_blob_kzg_proof(blob: Blob, commitment_bytes: &Bytes48, proof_bytes: &Bytes48, kzg_settings: &KzgSettings) -> Result<bool, KzgError> {
        let mut ok = false;
        ffi::check(unsafe { ffi::kzg_verify_blob_kzg_proof(&mut ok, blob.0.as_ptr(), commitment_bytes.0.as_ptr(), proof_bytes.0.as_ptr(), kzg_settings.raw()) })?;
        Ok(ok)
    }

    /// kzg-rs `src/kzg_proof.rs:472-525`, including the order of its early returns (empty -> `Ok(true)` and the
    /// single-blob shortcut come BEFORE the length checks, `:478-501`).  `Blob`, `Bytes48` are `repr(transparent)` byte
    /// arrays, so the three `Vec`s are handed over as they lie in memory.
    pub fn verify_blob_kzg_proof_batch(
        blobs: Vec<Blob>,
        commitments_bytes: Vec<Bytes48>,
        proofs_bytes: Vec<Bytes48>,
        kzg_settings: &KzgSettings,
    ) -> Result<bool, KzgError> {
        if blobs.is_empty() {
            return Ok(true);
        }
        if blobs.len() == 1 {
            return Self::verify_blob_kzg_proof(blobs[0].clone(), &commitments_bytes[0], &proofs_bytes[0], kzg_settings);
        }
        if blobs.len() != commitments_bytes.len() {
            return Err(KzgError::InvalidBytesLength("Invalid commitments length".to_string()));
        }
        if blobs.len() != proofs_bytes.len() {
            return Err(KzgError::InvalidBytesLength("Invalid proofs length".to_string()));
        }
        let mut ok = false;
        ffi::check(unsafe {
            ffi::kzg_verify_blob_kzg_proof_batch(
                &mut ok,
                blobs.as_ptr().cast::<u8>(),
                commitments_bytes.as_ptr().cast::<u8>(),
                proofs_bytes.as_ptr().cast::<u8>(),
                blobs.len(),
                kzg_settings.raw(),
            )
        })?;
        Ok(ok)
    }

    /// c-kzg-4844's `verify_cell_kzg_proof_batch` (EIP-7594; not in kzg-rs): one entry per cell - its blob's commitment, its
    /// cell index (< 128), the cell and its proof - checked with one random linear combination and one pairing
    /// (include/kzg_rs_amd.h).  Slices of unequal length are `InvalidBytesLength`; a cell index >= 128, a non-canonical field
    /// element or a point outside G1 is `BadArgs`; an empty batch is `Ok(true)`.
    pub fn verify_cell_kzg_proof_batch(
        commitments: &[Bytes48],
        cell_indices: &[u64],
        cells: &[Cell],
        proofs: &[Bytes48],
        kzg_settings: &KzgSettings,
    ) -> Result<bool, KzgError> {
        let n = cells.len();
        if commitments.len() != n || cell_indices.len() != n || proofs.len() != n {
            return Err(KzgError::InvalidBytesLength("commitments, cell indices, cells and proofs differ in length".to_string()));
        }
        let mut ok = false;
        ffi::check(unsafe {
            ffi::kzg_verify_cell_kzg_proof_batch(
                &mut ok,
                commitments.as_ptr().cast::<u8>(),
                cell_indices.as_ptr(),
                cells.as_ptr().cast::<u8>(),
                proofs.as_ptr().cast::<u8>(),
                n,
                kzg_settings.raw(),
            )
        })?;
        Ok(ok)
    }

    /// Blobs against their 128 cell proofs each, without computing a cell (not in kzg-rs; include/kzg_rs_amd.h): the Fulu check of
    /// a blob transaction's network wrapper and of `engine_getBlobsV2` answers.  `cell_proofs` holds the 128 proofs of blob 0,
    /// then those of blob 1, ...  Entry b is what `verify_cell_kzg_proof_batch` returns for blob b's commitment x 128, the cell
    /// indices 0..127, its cells and its proofs: `Ok(verdict)`, or `BadArgs` for a non-canonical field element or a point
    /// outside G1 - the other blobs keep their own results.  Slices whose lengths do not fit are `InvalidBytesLength`.
    pub fn verify_blob_cell_kzg_proofs(
        blobs: &[Blob],
        commitments: &[Bytes48],
        cell_proofs: &[Bytes48],
        kzg_settings: &KzgSettings,
    ) -> Result<Vec<Result<bool, KzgError>>, KzgError> {
        let n = blobs.len();
        if commitments.len() != n || cell_proofs.len() != 128 * n {
            return Err(KzgError::InvalidBytesLength("every blob needs one commitment and 128 cell proofs".to_string()));
        }
        let mut ok = vec![false; n];
        let mut err = vec![0u8; n];
        ffi::check(unsafe {
            ffi::kzg_verify_blob_cell_kzg_proofs(
                ok.as_mut_ptr(),
                err.as_mut_ptr(),
                blobs.as_ptr().cast::<u8>(),
                commitments.as_ptr().cast::<u8>(),
                cell_proofs.as_ptr().cast::<u8>(),
                n,
                kzg_settings.raw(),
            )
        })?;
        Ok((0..n)
            .map(|b| if err[b] != 0 { Err(KzgError::BadArgs("a field element >= r or a point outside G1".to_string())) } else { Ok(ok[b]) })
            .collect())
    }

    /// c-kzg-4844's `compute_cells` (EIP-7594; not in kzg-rs): the 128 cells of every blob, blob after blob
    /// (include/kzg_rs_amd.h).  A field element >= r is `BadArgs`.
    pub fn compute_cells(blobs: &[Blob], kzg_settings: &KzgSettings) -> Result<Vec<Cell>, KzgError> {
        let n = blobs.len();
        let mut cells: Vec<u8> = alloc::vec![0u8; n * 128 * crate::dtypes::BYTES_PER_CELL];
        ffi::check(unsafe { ffi::kzg_compute_cells(cells.as_mut_ptr(), blobs.as_ptr().cast::<u8>(), n, kzg_settings.raw()) })?;
        cells.chunks_exact(crate::dtypes::BYTES_PER_CELL).map(Cell::from_slice).collect()
    }

    /// c-kzg-4844's `compute_cells_and_kzg_proofs`: the same cells and the 128 proofs of every blob (FK20 on the device).
    pub fn compute_cells_and_kzg_proofs(blobs: &[Blob], kzg_settings: &KzgSettings) -> Result<(Vec<Cell>, Vec<Bytes48>), KzgError> {
        let n = blobs.len();
        let mut cells: Vec<u8> = alloc::vec![0u8; n * 128 * crate::dtypes::BYTES_PER_CELL];
        let mut proofs: Vec<u8> = alloc::vec![0u8; n * 128 * 48];
        ffi::check(unsafe {
            ffi::kzg_compute_cells_and_kzg_proofs(cells.as_mut_ptr(), proofs.as_mut_ptr(), blobs.as_ptr().cast::<u8>(), n, kzg_settings.raw())
        })?;
        let cells: Result<Vec<Cell>, KzgError> = cells.chunks_exact(crate::dtypes::BYTES_PER_CELL).map(Cell::from_slice).collect();
        let proofs: Result<Vec<Bytes48>, KzgError> = proofs.chunks_exact(48).map(Bytes48::from_slice).collect();
        Ok((cells?, proofs?))
    }

    /// c-kzg-4844's `recover_cells_and_kzg_proofs` for one blob: all 128 cells and proofs from at least 64 of its cells, the
    /// indices strictly ascending (include/kzg_rs_amd.h).  Slices of unequal length are `InvalidBytesLength`; fewer than 64 or
    /// more than 128 cells, an index >= 128, a non-canonical field element and cells that lie on no polynomial of degree < 4096
    /// are `BadArgs`.
    pub fn recover_cells_and_kzg_proofs(cell_indices: &[u64], cells: &[Cell], kzg_settings: &KzgSettings) -> Result<(Vec<Cell>, Vec<Bytes48>), KzgError> {
        if cell_indices.len() != cells.len() {
            return Err(KzgError::InvalidBytesLength("cell indices and cells differ in length".to_string()));
        }
        let mut out: Vec<u8> = alloc::vec![0u8; 128 * crate::dtypes::BYTES_PER_CELL];
        let mut proofs: Vec<u8> = alloc::vec![0u8; 128 * 48];
        ffi::check(unsafe {
            ffi::kzg_recover_cells_and_kzg_proofs(
                out.as_mut_ptr(),
                proofs.as_mut_ptr(),
                cell_indices.as_ptr(),
                cells.as_ptr().cast::<u8>(),
                cells.len(),
                1,
                kzg_settings.raw(),
            )
        })?;
        let out: Result<Vec<Cell>, KzgError> = out.chunks_exact(crate::dtypes::BYTES_PER_CELL).map(Cell::from_slice).collect();
        let proofs: Result<Vec<Bytes48>, KzgError> = proofs.chunks_exact(48).map(Bytes48::from_slice).collect();
        Ok((out?, proofs?))
    }

    /// The same recovery for a caller that also holds the KZG proof of every given cell and HAS VERIFIED those pairs
    /// (`kzg_recover_cells_and_kzg_proofs_given_proofs`, include/kzg_rs_amd.h): the missing proofs are interpolated from the first 64
    /// given ones instead of being recomputed by FK20.  The proofs are not checked against the cells: with wrong but well-formed
    /// proofs the call succeeds and the missing proofs are wrong.  A given proof that is not a G1 point is `BadArgs`.
    pub fn recover_cells_and_kzg_proofs_given_proofs(
        cell_indices: &[u64],
        cells: &[Cell],
        proofs: &[Bytes48],
        kzg_settings: &KzgSettings,
    ) -> Result<(Vec<Cell>, Vec<Bytes48>), KzgError> {
        if cell_indices.len() != cells.len() || proofs.len() != cells.len() {
            return Err(KzgError::InvalidBytesLength("cell indices, cells and proofs differ in length".to_string()));
        }
        let mut out: Vec<u8> = alloc::vec![0u8; 128 * crate::dtypes::BYTES_PER_CELL];
        let mut all: Vec<u8> = alloc::vec![0u8; 128 * 48];
        ffi::check(unsafe {
            ffi::kzg_recover_cells_and_kzg_proofs_given_proofs(
                out.as_mut_ptr(),
                all.as_mut_ptr(),
                cell_indices.as_ptr(),
                cells.as_ptr().cast::<u8>(),
                proofs.as_ptr().cast::<u8>(),
                cells.len(),
                1,
                kzg_settings.raw(),
            )
        })?;
        let out: Result<Vec<Cell>, KzgError> = out.chunks_exact(crate::dtypes::BYTES_PER_CELL).map(Cell::from_slice).collect();
        let all: Result<Vec<Bytes48>, KzgError> = all.chunks_exact(48).map(Bytes48::from_slice).collect();
        Ok((out?, all?))
    }
}
