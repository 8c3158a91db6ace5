// Proof::verify on proof bytes that sit in device memory (rv_verify_device, rv_verify_sections_device; verify_dev.inc drives it).
//
// The host verifier parses the proof, builds the slot arrays (verify.inc: check_records, fill_slots) and uploads them with the
// online records.  Here the proof stays where it is: ONE walk over its framing (walk_proof, below: the same function on the host
// and in k_parse_proof) leaves a table of where every record's parts are, k_fill_slots_dev writes the slot arrays from that table,
// and the unpack kernels read the vectors in place (src offsets from the proof's first byte).
//
// walk_proof is plain C++ without a HIP construct outside the RV_VW_HD marker, so that a host program can include this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RV_VW_HD __host__ __device__
#else
#define RV_VW_HD
#endif

namespace rv {

// how the bytes are framed
constexpr int VW_FRAMING_PROOF = 0;     // bincode(Proof): comm | per domain: u64 40, 40 records, u64 216, 216 x 48 bytes; bytes behind it are ignored
constexpr int VW_FRAMING_SECTIONS = 1;  // [gf2 records | gf2 preprocessing | z64 records | z64 preprocessing], lens[4]: no comm, no counts

// what the walk ends with; everything but VW_OK sends the call to the host verifier (which then gives the reference's answer)
constexpr int VW_OK = 0;
constexpr int VW_SHORT = 1;    // the bytes run out inside a field
constexpr int VW_COUNT = 2;    // a repetition count is not 40 / 216 (found before a single record of that count is walked)
constexpr int VW_SECTION = 3;  // sections: a section's records do not end on its end, a preprocessing section is not 216 x 48 bytes
constexpr int VW_RECORDS = 4;  // check_records' rules refuse a group (verify.inc)

// The table, in 64-bit words.  Record k = 40 * domain + i (domain 0 GF(2), 1 Z64; i the record's place among the 40) has eight
// words at VW_REC + 8 * k: the offsets of its keys, rec, corr and in bytes from the first byte walked, the three lengths, its omit
// byte.  The tail -- status, the 80 omit bytes, comm -- is one block, so that it goes to the host in one small copy.
constexpr int VW_N_ON = 40, VW_N_PRE = 216;
constexpr int VW_KEYS = 0, VW_OFF_REC = 1, VW_LEN_REC = 2, VW_OFF_CORR = 3, VW_LEN_CORR = 4, VW_OFF_IN = 5, VW_LEN_IN = 6, VW_REC_OMIT = 7;
constexpr int VW_REC = 0;                           // [80][8]
constexpr int VW_PRE = VW_REC + 8 * 2 * VW_N_ON;    // [2]: where a domain's 216 x (seed[16] | comm_online[32]) start
constexpr int VW_STATUS = VW_PRE + 2;               // [1]
constexpr int VW_OMIT = VW_STATUS + 1;              // 80 bytes (record k's at byte k), 10 words
constexpr int VW_COMM = VW_OMIT + 2 * VW_N_ON / 8;  // 32 bytes, 4 words (sections: zero)
constexpr int VW_WORDS = VW_COMM + 4;
constexpr int VW_HEAD = VW_STATUS, VW_HEAD_WORDS = VW_WORDS - VW_STATUS;  // what the host reads back

// n bytes at *pos of [0, end): false when they are not there, else *at = their offset and *pos moves on.  pos <= end always, so
// end - pos cannot wrap, and n is compared before anything is added (Reader::take, verify.inc).
RV_VW_HD inline bool vw_take(uint64_t* pos, uint64_t end, uint64_t n, uint64_t* at) {
    if (n > end - *pos) return false;
    *at = *pos;
    *pos += n;
    return true;
}
RV_VW_HD inline bool vw_u64(const uint8_t* p, uint64_t* pos, uint64_t end, uint64_t* v) {
    uint64_t at;
    if (!vw_take(pos, end, 8, &at)) return false;
    uint64_t x = 0;
    for (int i = 0; i < 8; i++) x |= (uint64_t)p[at + i] << (8 * i);
    *v = x;
    return true;
}

// Walks p[0, len) and fills table[VW_WORDS] (the words behind a stop are not written; table[VW_STATUS] always is).  lens: the
// four section lengths (VW_FRAMING_SECTIONS; their sum must be len -- the caller checks that), ignored for a bincode proof.
// Every byte is loaded only after vw_take has found it inside [0, len), and inside its section where there are sections.
RV_VW_HD inline int walk_proof(const uint8_t* p, uint64_t len, int framing, const uint64_t* lens, uint64_t* table) {
    const bool sections = framing == VW_FRAMING_SECTIONS;
    uint8_t* omits = (uint8_t*)(table + VW_OMIT);
    uint64_t pos = 0, at = 0;
    int status = VW_OK;
    for (int i = 0; i < 4; i++) table[VW_COMM + i] = 0;
    if (!sections) {
        if (!vw_take(&pos, len, 32, &at)) status = VW_SHORT;
        else
            for (int i = 0; i < 32; i++) ((uint8_t*)(table + VW_COMM))[i] = p[at + i];
    }
    for (int dom = 0; dom < 2 && status == VW_OK; dom++) {
        uint64_t end = len, n = 0;
        if (sections) {
            if (lens[2 * dom] > len - pos) {
                status = VW_SECTION;
                break;
            }
            end = pos + lens[2 * dom];
        } else {
            if (!vw_u64(p, &pos, end, &n)) status = VW_SHORT;
            else if (n != VW_N_ON) status = VW_COUNT;
        }
        for (int i = 0; i < VW_N_ON && status == VW_OK; i++) {
            uint64_t* rec = table + VW_REC + 8 * (VW_N_ON * dom + i);
            bool ok = vw_take(&pos, end, 1, &at);
            if (ok) {
                rec[VW_REC_OMIT] = p[at];
                omits[VW_N_ON * dom + i] = p[at];
            }
            ok = ok && vw_take(&pos, end, 128, &rec[VW_KEYS]);
            ok = ok && vw_u64(p, &pos, end, &rec[VW_LEN_REC]) && vw_take(&pos, end, rec[VW_LEN_REC], &rec[VW_OFF_REC]);
            ok = ok && vw_u64(p, &pos, end, &rec[VW_LEN_CORR]) && vw_take(&pos, end, rec[VW_LEN_CORR], &rec[VW_OFF_CORR]);
            ok = ok && vw_u64(p, &pos, end, &rec[VW_LEN_IN]) && vw_take(&pos, end, rec[VW_LEN_IN], &rec[VW_OFF_IN]);
            if (!ok) status = VW_SHORT;
        }
        if (status != VW_OK) break;
        if (sections) {
            if (pos != end || lens[2 * dom + 1] != (uint64_t)VW_N_PRE * 48) status = VW_SECTION;
        } else {
            if (!vw_u64(p, &pos, len, &n)) status = VW_SHORT;
            else if (n != VW_N_PRE) status = VW_COUNT;
        }
        if (status == VW_OK && !vw_take(&pos, len, (uint64_t)VW_N_PRE * 48, &table[VW_PRE + dom])) status = VW_SHORT;
    }
    // check_records (verify.inc) for the five online groups: an omit byte of 8 or more in either domain; in a GF(2) group a rec
    // length that differs from the first record's, a corr or in length below it
    for (int k = 0; k < 2 * VW_N_ON && status == VW_OK; k++)
        if (omits[k] >= 8) status = VW_RECORDS;
    for (int i = 0; i < VW_N_ON && status == VW_OK; i++) {
        const uint64_t* o = table + VW_REC + 8 * i;
        const uint64_t* o0 = table + VW_REC + 8 * (i & ~7);
        if (o[VW_LEN_REC] != o0[VW_LEN_REC] || o[VW_LEN_CORR] < o0[VW_LEN_CORR] || o[VW_LEN_IN] < o0[VW_LEN_IN]) status = VW_RECORDS;
    }
    table[VW_STATUS] = (uint64_t)status;
    return status;
}

#if defined(__HIPCC__)
// the device arrays k_fill_slots_dev writes: verify.inc's SlotArrays for the verifier's 256 slots in slot order (0 .. 39 the online
// records, 40 .. 255 the preprocessing ones)
struct DevSlotArrays {
    uint8_t *seeds, *omit, *hkeys, *hco, *hco64;  // [256][16], [256], [256][128], [256][32], [256][32]
    uint32_t *keep, *onm;                          // [64] each
    uint64_t* src;                                 // [6][256]
    uint8_t *seeds64, *omit64, *hkeys64;           // the Z64 side (has64 only)
    uint32_t* keep64;
    uint64_t* src64;
};
// k_parse_proof on `st`: walk_proof over d_bytes[0, len) into d_table[VW_WORDS]; d_lens: the four section lengths in device
// memory (sections) or null.  head_mapped (nullable): device address of page-locked host memory that receives the table's tail.
void launch_parse_proof(hipStream_t st, const uint8_t* d_bytes, uint64_t len, int framing, const uint64_t* d_lens, uint64_t* d_table,
                        uint64_t* head_mapped);
// k_fill_slots_dev on `st`: what fill_slots makes of a proof that walked to VW_OK, for groups 0 .. 31 at base offset 0
void launch_fill_slots_dev(hipStream_t st, const uint8_t* d_bytes, const uint64_t* d_table, bool has64, const DevSlotArrays& a);

// ---- the same for the proofs of a batch (rv_verify_batch_device, batch_dev.inc)
// one proof of a batch: its bytes in device memory and, for the fill kernel, its table
struct BatchProofRef {
    const uint8_t* bytes;
    uint64_t len;
    const uint64_t* table;
};
// byte offsets of the slot arrays inside a proof's slot of the batch verifier's slab (verify_batch.inc: Slot), slots `stride` apart
struct BatchSlotLayout {
    uint64_t seeds, omit, keep, onm, quads, hkeys, hco, hco64, src, seeds64, omit64, keep64, hkeys64, src64, stride;
};
// k_parse_proofs on `st`: one wavefront per proof (blockIdx.x), lane 0 runs walk_proof over d_refs[b].bytes[0, len) into
// d_tables[b][VW_WORDS]; heads[b][VW_HEAD_WORDS] (device memory, or the device address of mapped host memory) receives the
// table's tail, zeros behind the status of a walk that stopped
void launch_parse_proofs(hipStream_t st, const BatchProofRef* d_refs, uint32_t batch, uint64_t* d_tables, uint64_t* heads);
// k_fill_slots_batch on `st`: k_fill_slots_dev's values for live proof k (gridDim.y) into d_slab + k * L.stride at L's offsets
// (src offsets from the proof's own first byte), and the opened quad words 0 .. 9 into L.quads
void launch_fill_slots_batch(hipStream_t st, const BatchProofRef* d_refs, uint32_t n_live, uint8_t* d_slab, const BatchSlotLayout& L, bool has64);
#endif

}  // namespace rv
