// link_supertig -- the link_scaffold module's long-read linker (link_scaffold/link_supertig.cpp + link_func.cpp) with the link table,
// the gap statistics, the slices of the reads that span every gap and the super-contig sequences computed on the GPU (SUPER section
// of include/dbgk.h).  Same command line, same seven output files <prefix>.supertig.{links.all,links.uniq,seq.fa,pos.tab,gap.data}
// and .supertig_repeat.{seq.fa,pos.tab}, same protocol on stderr.
#include <algorithm>
#include <unordered_map>

#include "link_common.h"

static void usage()
{
	cerr << "\nlink_supertig  <contig|scafftig_file.fa>  <mapping_twoctg_files.lib>\n"
	     << "   Function: link illumina-derived scafftigs into super-contigs by pacbio reads, inside gap are filled" << endl
	     << "   Version: 1.0" << endl
	     << "   -n <int>   the minimum number of read-ends required to support a link, default=" << PairNumCut << endl
	     << "   -o <str>   the output prefix, set in commond-line, default = " << Output_prefix << endl
	     << "   -h         get the help information\n" << endl
	     << "Example:    link_supertig Ecoli.scafftig.seq.fa  pacbio_mapping.lib\n" << endl;
	exit(0);
}

static void output_parameters()
{
	cerr << "link_supertig   [version 1.0]" << endl
	     << "   -n <int>   the minimum number of read-ends required to support a link, default=" << PairNumCut << endl
	     << "   -o <str>   the output prefix, set in commond-line, default = " << Output_prefix << endl
	     << "   -h         get the help information\n" << endl;
}

// ReadsInfo (link_supertig.cpp:243-248): the reads of the .reads.fa.gz files by id.  A read only the map files name gets an index
// behind those of the reads that are there, which the device call refuses when a gap needs it.
struct Reads {
	unordered_map<string, int32_t> index;
	vector<string> seqs;                       // the reads that are there
	vector<string> absent;                     // ids only the map files name, index seqs.size() + position
	unordered_map<string, int32_t> absent_index;
	int32_t id_of(const string &name)
	{
		auto it = index.find(name);
		if (it != index.end()) return it->second;
		it = absent_index.find(name);
		if (it != absent_index.end()) return it->second;
		const int32_t id = (int32_t)(seqs.size() + absent.size());
		absent_index.emplace(name, id);
		absent.push_back(name);
		return id;
	}
	const string &name_of(int64_t id) const
	{
		static const string unknown = "?";
		if (id >= (int64_t)seqs.size()) return id - seqs.size() < absent.size() ? absent[id - seqs.size()] : unknown;
		for (const auto &kv : index)
			if (kv.second == id) return kv.first;
		return unknown;
	}
};

// load_reads_fa_file (link_supertig.cpp:646-667): a later entry of an id replaces an earlier one
static bool load_reads_fa_file(const string &file, Reads &reads)
{
	LineReader in(file, false);
	if (!in.ok()) return false;
	string line, seq;
	vector<string> v;
	while (in.getline(line)) {
		if (line.empty() || line[0] != '>') continue;
		v.clear();
		split(line, v, "> \t\n");
		in.getline(seq);
		if (v.empty()) continue;
		auto it = reads.index.find(v[0]);
		if (it != reads.index.end()) {
			reads.seqs[it->second] = seq;
		} else {
			reads.index.emplace(v[0], (int32_t)reads.seqs.size());
			reads.seqs.push_back(seq);
		}
	}
	return true;
}

// the fields parse_read_ends_map_file (link_func.cpp:167-173) and load_map_twoctg_file (link_supertig.cpp:611-643) take from one line
static void parse_map_file(const string &file, dbgk_super *L, size_t n_contigs, Reads &reads)
{
	LineReader in(file);
	vector<dbgk_fill_record> batch;
	batch.reserve(BatchRecords);
	auto flush = [&]() {
		const int rc = dbgk_super_add_records(L, batch.data(), batch.size());
		if (rc) die("dbgk_super_add_records", rc);
		batch.clear();
	};
	string line;
	vector<string> v;
	int id1 = 0, id2 = 0;
	while (in.getline(line)) {
		if (!split_map_line("link_supertig", file, line, n_contigs, v, id1, id2)) continue;
		if (id1 == id2) { // map_reads never writes such a line
			cerr << "link_supertig: a line of " << file << " has both ends of " << v[0] << " on " << v[4] << endl;
			exit(1);
		}
		dbgk_fill_record r{};
		r.read = reads.id_of(v[0]);
		r.read_len = atoi(v[1].c_str());
		r.align1_end = atoi(v[3].c_str());
		r.align2_start = atoi(v[12].c_str());
		r.contig1 = id1 / 2;
		r.contig2 = id2 / 2;
		r.direct1 = v[8].size() == 1 ? (uint8_t)v[8][0] : (uint8_t)'?';
		r.direct2 = v[18].size() == 1 ? (uint8_t)v[18][0] : (uint8_t)'?';
		batch.push_back(r);
		if (batch.size() >= BatchRecords) flush();
	}
	flush();
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "n:o:h")) != -1) {
		switch (c) {
			case 'n': PairNumCut = atoi(optarg); break;
			case 'o': Output_prefix = optarg; break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 3 || argc - optind < 2) usage(); // (the reference reads argv past its end when options leave fewer than two names)
	output_parameters();
	const string contig_seq_file = argv[optind++];
	const string para_map_file = argv[optind++];

	const clock_t time_start = clock();
	auto run_time = [&]() { cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl; };
	cerr << "\nProgram start ............" << endl;
	run_time();

	vector<string> contig_ids, contig_seqs;
	vector<uint32_t> lens;
	uint64_t contig_total_len = 0;
	load_contigs("link_supertig", contig_seq_file, contig_ids, contig_seqs, lens, contig_total_len);
	const size_t n_contigs = contig_seqs.size();

	vector<string> Paired_map_files;
	reading_lib_file(para_map_file, Paired_map_files);
	cerr << "\nInput reads mapping files number: " << Paired_map_files.size() << endl;
	run_time();

	dbgk_super *L = nullptr;
	dbgk_super_params P{PairNumCut, {0, 0, 0}};
	int rc = dbgk_super_create(&P, 0, &L);
	if (rc) die("dbgk_super_create", rc);
	if ((rc = dbgk_super_set_contigs(L, lens.data(), n_contigs))) die("dbgk_super_set_contigs", rc);

	// the reads come first here, so that a record can name its read by index (the reference loads them behind the passes; its
	// messages keep their place below)
	Reads reads;
	vector<bool> reads_file_ok;
	for (size_t i = 0; i < Paired_map_files.size(); i++) reads_file_ok.push_back(load_reads_fa_file(Paired_map_files[i] + ".reads.fa.gz", reads));
	{
		string bases;
		vector<uint64_t> offsets;
		concat(reads.seqs, bases, offsets);
		if ((rc = dbgk_super_set_reads(L, bases.data(), offsets.data(), reads.seqs.size()))) die("dbgk_super_set_reads", rc);
	}
	for (size_t i = 0; i < Paired_map_files.size(); i++) {
		cerr << "\nparse map file: " << Paired_map_files[i] << endl;
		parse_map_file(Paired_map_files[i], L, n_contigs, reads);
	}
	if ((rc = dbgk_super_build(L))) {
		if (rc == DBGK_ERR_ARG) cerr << "link_supertig: the gaps of one contig pair sum to more than an int holds" << endl;
		die("dbgk_super_build", rc);
	}
	cerr << "\nParsed the map files done !" << endl;
	run_time();

	const size_t n_nodes = 2 * n_contigs + 1;
	vector<uint64_t> first(n_nodes + 1);
	uint64_t n_links = 0;
	dbgk_link_counters ctr{};
	if ((rc = dbgk_super_export(L, first.data(), nullptr, 0, &n_links, &ctr))) die("dbgk_super_export", rc);
	report_link_classes(ctr);

	dbgk_super_summary S{};
	if ((rc = dbgk_super_resolve(L, &S))) {
		if (rc == DBGK_ERR_ARG && S.bad_read >= 0)
			cerr << "link_supertig: read " << reads.name_of(S.bad_read) << " that spans " << contig_ids[S.bad_left] << " and " << contig_ids[S.bad_right]
			     << " is missing from the .reads.fa.gz files or too short for the slice around its gap" << endl;
		die("dbgk_super_resolve", rc);
	}
	cerr << "\nRemoved LowFreq link num: " << S.lowfreq << endl;
	auto snapshot = [&](int stage, uint8_t *inlink, uint8_t *link, dbgk_link_entry *e) {
		if (int rc = dbgk_super_snapshot(L, stage, inlink, link, e)) die("dbgk_super_snapshot", rc);
	};
	report_3prime_links(snapshot, n_nodes);
	const string stem = Output_prefix + ".supertig";
	display_data_in_link(snapshot, 0, first, stem + ".links.all");
	cerr << "\nRemoved interleave links num: " << S.interleave << endl;
	cerr << "\nRemoved repeat nodes num: " << S.repeat_nodes << endl;
	cerr << "\nRemoved links [related with repeat or small nodes] num: " << S.deleted << endl;
	display_data_in_link(snapshot, 1, first, stem + ".links.uniq");
	for (size_t i = 0; i < Paired_map_files.size(); i++) {
		cerr << "\nparse reads file: " << Paired_map_files[i] << ".reads.fa.gz" << endl;
		if (!reads_file_ok[i]) cerr << "fail to open input file " << Paired_map_files[i] << ".reads.fa.gz" << endl;
	}
	cerr << "load reads used to fill gaps done\n" << endl;
	for (size_t i = 0; i < Paired_map_files.size(); i++) cerr << "\nparse map file: " << Paired_map_files[i] << endl;
	cerr << "load reads mapping results done\n" << endl;
	cerr << "Decide the gap sizes done\n" << endl;

	// fill_gaps_inside_scaffold (link_supertig.cpp:333-558): the layout comes sorted, the sequences of all super-contigs from one
	// device call, the slices of all gaps from another
	vector<uint64_t> scaf_first(S.scaffolds + 1);
	vector<dbgk_link_item> items(S.items + 1);
	vector<dbgk_super_junction> junctions(S.junctions + 1);
	vector<int32_t> repeats(S.repeat_nodes + 1);
	if ((rc = dbgk_super_layout(L, scaf_first.data(), items.data(), junctions.data(), repeats.data()))) die("dbgk_super_layout", rc);
	vector<dbgk_super_slice> slices(S.slices + 1);
	uint64_t n_slices = 0, n_slice_bytes = 0;
	if ((rc = dbgk_super_slices(L, slices.data(), slices.size(), &n_slices))) die("dbgk_super_slices", rc);
	string slice_bytes(S.slice_bytes, '\0');
	if ((rc = dbgk_super_slice_bytes(L, &slice_bytes[0], slice_bytes.size(), &n_slice_bytes))) die("dbgk_super_slice_bytes", rc);
	string bases;
	vector<uint64_t> offsets;
	concat(contig_seqs, bases, offsets);
	const string seq = emit_sequences([&](char *out, uint64_t capacity, uint64_t *out_len) {
		return dbgk_super_emit(L, bases.data(), offsets.data(), n_contigs, items.data(), S.items, out, capacity, out_len);
	}, "dbgk_super_emit");

	// *.supertig.gap.data and the messages of the gaps, in walk order (gap ids 1, 2, ...)
	{
		ofstream ScafGapFile((stem + ".gap.data").c_str());
		if (!ScafGapFile) cerr << "fail to open file" << stem + ".gap.data" << endl;
		vector<const dbgk_super_junction *> by_id(S.junctions);
		for (uint64_t j = 0; j < S.junctions; j++) by_id[junctions[j].gap_id - 1] = &junctions[j];
		uint64_t gap_reads_id = 1;
		for (const dbgk_super_junction *J : by_id) {
			if (J->mean <= 0) cerr << "Error may happens: mean_gap_size <= 0" << endl;
			const dbgk_super_slice *sl = slices.data() + J->first_slice;
			const dbgk_super_slice &median = sl[J->median];
			ScafGapFile << ">gap" << J->gap_id << " length=" << median.length << " nodes=" << J->n_kept << "\n";
			ScafGapFile << "Y\tS" << gap_reads_id++ << "\t+\t0\t" << median.length << "\t";
			ScafGapFile.write(slice_bytes.data() + median.offset, median.length);
			ScafGapFile << "\n";
			for (uint32_t k = 0; k < J->n_slices; k++) {
				if ((int32_t)k == J->median) continue;
				if (sl[k].kept) {
					ScafGapFile << "N\tS" << gap_reads_id++ << "\t+\t0\t" << sl[k].length << "\t";
					ScafGapFile.write(slice_bytes.data() + sl[k].offset, sl[k].length);
					ScafGapFile << "\n";
				} else {
					cerr << "Altert message:  gap_id " << J->gap_id << "  " << median.length << "\t" << sl[k].length << endl;
				}
			}
		}
	}

	ofstream ScafPosFile((stem + ".pos.tab").c_str());
	if (!ScafPosFile) cerr << "fail to open file" << stem + ".pos.tab" << endl;
	ofstream ScafSeqFile((stem + ".seq.fa").c_str());
	if (!ScafSeqFile) cerr << "fail to open file" << stem + ".seq.fa" << endl;
	uint64_t total_supertig_len = 0;
	ContigTally included;
	int supertig_id = -1;
	uint64_t seq_pos = 0, junction = 0;
	for (uint64_t s = 0; s < S.scaffolds; s++) {
		supertig_id += 2;
		int scaf_ctg_num = 0, scaf_len = 0;
		const uint64_t seq_begin = seq_pos;
		ScafPosFile << ">spt_" << supertig_id << "\n";
		for (uint64_t t = scaf_first[s]; t < scaf_first[s + 1]; t++) {
			const dbgk_link_item &it = items[t];
			const int block_start = scaf_len + 1;
			if (it.contig >= 0) {
				const int block_size = (int)lens[it.contig];
				scaf_ctg_num++;
				scaf_len += block_size;
				ScafPosFile << "\t" << contig_ids[it.contig] << "\t" << block_start << "\t" << scaf_len << "\t" << block_size << "\t" << (it.value ? "R" : "F")
				            << "\t";
				ScafPosFile.write(seq.data() + seq_pos, block_size);   // the oriented contig as the device wrote it
				ScafPosFile << "\n";
				seq_pos += (uint64_t)block_size;
				included.num++;
				included.len += block_size;
			} else {
				const dbgk_super_junction &J = junctions[junction++];
				scaf_len += it.value;
				seq_pos += (uint64_t)it.value;
				ScafPosFile << "\tgap" << J.gap_id << "\t" << block_start << "\t" << scaf_len << "\t" << it.value << "\tN\t" << J.min << "\t" << J.max << "\t"
				            << J.total << "\t" << J.variance << "\n";
			}
		}
		ScafSeqFile << ">spt_" << supertig_id << "   fragment_num:" << scaf_ctg_num << "   length:" << scaf_len << "   lenwogap:" << scaf_len << "\n";
		ScafSeqFile.write(seq.data() + seq_begin, scaf_len);
		ScafSeqFile << "\n";
		total_supertig_len += scaf_len;
	}
	ScafPosFile.close();
	ScafSeqFile.close();
	cerr << "\nFill gaps inside scaffold sequence done" << endl;

	const ContigTally excluded = write_repeat_contigs(Output_prefix + ".supertig_repeat", "spt_", supertig_id, repeats, S.repeat_nodes, contig_ids,
	                                                  contig_seqs, lens);

	cerr << "\nTotal supertig number:          " << S.scaffolds << endl;
	cerr << "Total supertig length[WithGap]: " << total_supertig_len << endl;
	cerr << "Total supertig length[NoGap]:   " << total_supertig_len << endl;
	report_contig_use(included, excluded, n_contigs, contig_total_len);
	cerr << "\nProgram finished !" << endl;
	run_time();
	dbgk_super_destroy(L);
	return 0;
}
